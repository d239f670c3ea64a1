// kernels_zi.hip.h -- device side of the zero-inflated GP / NB stage (ops_zi.hip): the E-step, M-step and soft imputation the
// reference's CPU fit runs after every dispersion update (inst/include/FactorNet/nmf/fit_cpu.hpp:1285-1552), over the entries the
// CSC does NOT store.  fp64, sparse input, ZI mode ROW or COL.  (fp32, dense input, masks, cross-validation and several devices
// are out of scope: the entries refuse them.)
//
//   bitmask_kernel            one bit per (i, j), set where the CSC stores an entry: word (tr, j) holds rows 64 tr .. 64 tr + 63 of
//                             column j, at bits[tr * n + j] -- the 64 words of a tile are contiguous.  One thread per column, plain
//                             stores (a word belongs to one column)
//   scatter_stored_kernel     A_imputed(i, j) = A_imputed^T(j, i) = x at the stored entries, once per fit: the impute kernel never
//                             writes there, so the stored entries stay bitwise A's
//   zi_estep_kernel<LOSS, MODE>  s = max((W_T o d)_i . h_j, 1e-10) a 64 x 64 tile at a time (the tile of kernels_distribution.hip.h:
//                             panels of 16 factors in LDS, an FMA chain in factor order), p0, z at the unstored entries; per-tile row
//                             (ROW) or column (COL) partials of z: the thread's 4 entries in order, then the 16 thread groups in
//                             order.  zi_sum_partials_kernel adds the tile partials in tile order
//   zi_mstep_kernel           pi = clamp(zsum / extent, 0.001, 0.999) where the row / column has an unstored entry; the GP theta floor
//   zi_impute_kernel<LOSS, MODE> the same tile with the updated pi (the factor product is recomputed, not parked by the E-step);
//                             z s goes to an LDS tile and leaves from there twice: as runs of 64 rows into A_imputed (column-major
//                             m x n) and as runs of 64 columns into A_imputed^T (column-major n x m)
//
// No floating-point atomics.  A tile's result depends on (m, n, k) alone: the kernels walk the tiles with a grid-stride loop, so the
// number of workgroups launched changes nothing.  All indices into m x n arrays are 64-bit.
#pragma once
#include "kernels.hip.h"

namespace rzi {

constexpr int TM = 64, TN = 64, KC = 16, NT = 256;          // the tile of kernels_distribution.hip.h

enum { LOSS_GP = 4, LOSS_NB = 5 };
enum { MODE_ROW = 1, MODE_COL = 2 };

struct ZiArgs {
    const double* A;                     // k x m: a(f, i) = W_T(f, i) d_f
    const double* H;                     // k x n
    const double* disp;                  // m: NB size r_i / GP theta_i
    const double* pi;                    // m (ROW) or n (COL)
    const unsigned long long* bits;      // ntr x n words
    int64_t m, n;
    int k, ntr;
    int64_t ntiles;
    double* part;                        // E-step: ROW ntc x m, COL ntr x n
    double* imp;                         // impute: m x n column-major (may be NULL)
    double* impT;                        // impute: n x m column-major (may be NULL)
};

__global__ __launch_bounds__(NT) void bitmask_kernel(const int* __restrict__ colptr, const int* __restrict__ rowidx, int64_t m,
                                                     int64_t n, unsigned long long* __restrict__ bits) {
    const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    // rows strictly increasing within a column (checked by the entries): the words of a column are met in order
    int64_t cur = -1;
    unsigned long long w = 0ull;
    for (int e = colptr[j]; e < colptr[j + 1]; ++e) {
        const int64_t r = rowidx[e], tr = r >> 6;
        if (tr != cur) {
            if (cur >= 0) bits[cur * n + j] = w;
            cur = tr;
            w = 0ull;
        }
        w |= 1ull << (r & 63);
    }
    if (cur >= 0) bits[cur * n + j] = w;
}

// one wavefront per column over its stored entries
__global__ __launch_bounds__(NT) void scatter_stored_kernel(const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                            const double* __restrict__ vals, int64_t m, int64_t n,
                                                            double* __restrict__ imp, double* __restrict__ impT) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= n) return;
    for (int e = colptr[j] + lane; e < colptr[j + 1]; e += 64) {
        const int64_t r = rowidx[e];
        const double x = vals[e];
        if (imp) imp[j * m + r] = x;
        if (impT) impT[r * n + j] = x;
    }
}

// index arrays of the CSC that stores every entry of a rows x cols column-major array (column c = rows 0 .. rows - 1)
__global__ void full_index_kernel(int rows, int64_t cols, int* __restrict__ col_ptr, int* __restrict__ row_idx) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e <= cols) col_ptr[e] = (int)(e * rows);
    if (e < (int64_t)rows * cols) row_idx[e] = (int)(e % rows);
}

template <int LOSS>
__device__ __forceinline__ double zi_p0(double s, double dv) {
    if (LOSS == LOSS_NB) {
        const double r = fmax(dv, 1e-10);
        return pow(r / (r + s), r);
    }
    return exp(-s / (1.0 + dv));
}

// s of this thread's 4 x 4 entries of tile (tr, tc): rows r0 + tx + 16 i, columns c0 + ty + 16 j
__device__ __forceinline__ void zi_tile_product(const ZiArgs& a, int64_t r0, int64_t c0, double (*sA)[TM + 1], double (*sH)[TN + 1],
                                                double acc[4][4]) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int f0 = 0; f0 < a.k; f0 += KC) {
#pragma unroll
        for (int q = 0; q < (KC * TM) / NT; ++q) {
            const int idx = t + NT * q, r = idx / KC, f = idx % KC;
            const int64_t gi = r0 + r, gj = c0 + r;
            sA[f][r] = (gi < a.m && f0 + f < a.k) ? a.A[gi * a.k + f0 + f] : 0.0;
            sH[f][r] = (gj < a.n && f0 + f < a.k) ? a.H[gj * a.k + f0 + f] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < KC; ++f) {
            double av[4], hv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = sA[f][tx + 16 * i]; hv[i] = sH[f][ty + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], hv[j], acc[i][j]);
        }
        __syncthreads();
    }
}

template <int LOSS, int MODE>
__global__ __launch_bounds__(NT) void zi_estep_kernel(ZiArgs a) {
    __shared__ double sA[KC][TM + 1];
    __shared__ double sH[KC][TN + 1];
    __shared__ double red[16][TM + 1];
    __shared__ unsigned long long sBits[TN];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t tr = tile % a.ntr, tc = tile / a.ntr;
        const int64_t r0 = tr * TM, c0 = tc * TN;
        if (t < TN) sBits[t] = (c0 + t < a.n) ? a.bits[tr * a.n + c0 + t] : ~0ull;
        double acc[4][4];
        zi_tile_product(a, r0, c0, sA, sH, acc);          // (its barriers order sBits too)
        double z[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t gi = r0 + tx + 16 * i;
            const double dv = gi < a.m ? a.disp[gi] : 1.0;
            const double prow = (MODE == MODE_ROW && gi < a.m) ? a.pi[gi] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gj = c0 + ty + 16 * j;
                const bool zero = gi < a.m && gj < a.n && !((sBits[ty + 16 * j] >> (tx + 16 * i)) & 1ull);
                double v = 0.0;
                if (zero) {
                    const double s = fmax(acc[i][j], 1e-10);
                    const double p0 = zi_p0<LOSS>(s, dv);
                    const double p = MODE == MODE_ROW ? prow : a.pi[gj];
                    v = p / (p + (1.0 - p) * p0 + 1e-300);
                }
                z[i][j] = v;
            }
        }
        if (MODE == MODE_ROW) {
#pragma unroll
            for (int i = 0; i < 4; ++i) red[ty][tx + 16 * i] = ((z[i][0] + z[i][1]) + z[i][2]) + z[i][3];
            __syncthreads();
            if (t < TM && r0 + t < a.m) {
                double s = 0.0;
                for (int g = 0; g < 16; ++g) s += red[g][t];
                a.part[tc * a.m + r0 + t] = s;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[tx][ty + 16 * j] = ((z[0][j] + z[1][j]) + z[2][j]) + z[3][j];
            __syncthreads();
            if (t < TN && c0 + t < a.n) {
                double s = 0.0;
                for (int g = 0; g < 16; ++g) s += red[g][t];
                a.part[tr * a.n + c0 + t] = s;
            }
        }
        __syncthreads();                                    // red and sBits are rewritten by the next tile
    }
}

// out[i] = sum over tiles p (in order) of part[p * len + i]
__global__ __launch_bounds__(NT) void zi_sum_partials_kernel(const double* __restrict__ part, int64_t nparts, int64_t len,
                                                             double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= len) return;
    double s = 0.0;
    for (int64_t p = 0; p < nparts; ++p) s += part[p * len + i];
    out[i] = s;
}

// len = m (ROW) or n (COL); extent = n (ROW) or m (COL); zcnt = unstored entries per row / column.  theta (m) is floored for GP.
__global__ __launch_bounds__(NT) void zi_mstep_kernel(const double* __restrict__ zsum, const int* __restrict__ zcnt, int64_t len,
                                                      double extent, double* __restrict__ pi, double* __restrict__ theta, int64_t m,
                                                      double theta_min) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e < len && zcnt[e] > 0) pi[e] = fmin(fmax(zsum[e] / extent, 0.001), 0.999);
    if (theta && e < m && theta[e] < theta_min) theta[e] = theta_min;
}

template <int LOSS, int MODE>
__global__ __launch_bounds__(NT) void zi_impute_kernel(ZiArgs a) {
    __shared__ double sA[KC][TM + 1];
    __shared__ double sH[KC][TN + 1];
    __shared__ double tilev[TM][TN + 1];                    // [row][column]
    __shared__ unsigned long long sBits[TN];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int64_t tr = tile % a.ntr, tc = tile / a.ntr;
        const int64_t r0 = tr * TM, c0 = tc * TN;
        if (t < TN) sBits[t] = (c0 + t < a.n) ? a.bits[tr * a.n + c0 + t] : ~0ull;
        double acc[4][4];
        zi_tile_product(a, r0, c0, sA, sH, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t gi = r0 + tx + 16 * i;
            const double dv = gi < a.m ? a.disp[gi] : 1.0;
            const double prow = (MODE == MODE_ROW && gi < a.m) ? a.pi[gi] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gj = c0 + ty + 16 * j;
                const bool zero = gi < a.m && gj < a.n && !((sBits[ty + 16 * j] >> (tx + 16 * i)) & 1ull);
                double v = 0.0;
                if (zero) {
                    const double s = fmax(acc[i][j], 1e-10);
                    const double p0 = zi_p0<LOSS>(s, dv);
                    const double p = MODE == MODE_ROW ? prow : a.pi[gj];
                    v = (p / (p + (1.0 - p) * p0 + 1e-300)) * s;
                }
                tilev[tx + 16 * i][ty + 16 * j] = v;
            }
        }
        __syncthreads();
        // out: a wavefront writes 64 consecutive rows of one column (A_imputed), then 64 consecutive columns of one row (A_imputed^T);
        // stored entries (bit set) and everything outside the matrix are skipped
        const int lane = t & 63, w = t >> 6;
        if (a.imp) {
            const int64_t gi = r0 + lane;
            for (int c = w; c < TN; c += 4) {
                const int64_t gj = c0 + c;
                if (gi < a.m && gj < a.n && !((sBits[c] >> lane) & 1ull)) a.imp[gj * a.m + gi] = tilev[lane][c];
            }
        }
        if (a.impT) {
            const int64_t gj = c0 + lane;
            const unsigned long long wb = sBits[lane];
            for (int r = w; r < TM; r += 4) {
                const int64_t gi = r0 + r;
                if (gi < a.m && gj < a.n && !((wb >> r) & 1ull)) a.impT[gi * a.n + gj] = tilev[r][lane];
            }
        }
        __syncthreads();
    }
}

}  // namespace rzi
