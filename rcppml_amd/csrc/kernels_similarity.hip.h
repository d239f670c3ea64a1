// kernels_similarity.hip.h -- device side of the column-similarity entries (ops_similarity.hip): cosine() of sparse matrices and
// the batched cosines / Pearson correlations of factor matrices that align() needs (R/cosine.R, R/nmf_methods.R:261-271).  fp64.
//
// Sparse: C (nx x ny, column-major) = cosines of the columns of X (m x nx) against the columns of Y (m x ny), both CSC.
//   col_norm_kernel      one thread per column: the squares added in storage order (ascending row), unfused, then the square root
//   tile_offsets_kernel  X^T by rows (row r: the columns of X that store row r, ascending) cut into tiles of T columns:
//                        ts[t * m + r] = the first entry of row r at or past column t * T, t = 0 .. ntiles (binary search, once)
//   cosine_tile_kernel   one wavefront owns one (column j of Y, tile t of T columns of X) at a time and keeps that part of column j
//                        of C in LDS.  For each stored (r, v) of y_j in storage order its lanes walk the entries of row r of X^T
//                        that fall in the tile, acc[i] = acc[i] + v * x, unfused.  Within one row the i are distinct and the rows
//                        are issued in order by the same wavefront, so nothing conflicts and there is no atomic.  Then
//                        acc[i] / (|x_i| * |y_j|), 0 where a norm is 0, goes out with consecutive lanes on consecutive addresses.
//                        Every C[i, j] belongs to one item, items are dealt to wavefronts round-robin, and the order inside an item
//                        is fixed, so the result does not depend on the number of workgroups.
// With Y = X, C[i, j] and C[j, i] are the same chain: the same rows in the same order, products and the norm product commuted.
//
// Dense: reps matrices W_q (m x kx) against one R (m x ky), all column-major, kx, ky <= DK.
//   dense_stats_kernel   one wavefront per column: lane l adds rows l, l + 64, ..., then a butterfly over the 64 partials; the mean
//                        (method 1, 0 otherwise), then the norm of the centred column the same way
//   dense_partial_kernel one workgroup per (chunk of rows, replicate): the centred rows staged in LDS DSB at a time, a 16 x 16 thread
//                        grid with up to 8 x 8 pairs each, every pair an unfused chain over the chunk's rows in order
//   dense_final_kernel   chunk partials added in chunk order, divided by the norm product, 0 where a norm is 0
// The chunk length is a function of m alone (ops_similarity.hip), so the result does not depend on the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rsim {

constexpr int T = 2048;          // columns of X per LDS tile (16 KiB of fp64 per wavefront)
constexpr int WAVES = 8;         // wavefronts per workgroup: 128 KiB of the CU's 160 KiB, one workgroup per CU
constexpr int NT = WAVES * 64;
constexpr int DK = 128;          // most columns per side of the dense entry
constexpr int DSB = 16;          // rows per LDS stage of the dense kernel
constexpr int DNT = 256;

// Every product and sum below is rounded on its own: no operation of this file may be contracted into an FMA (the rounded
// operations are written out here, under the pragma, because contraction is decided where an operation is defined).
#pragma clang fp contract(off)
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }
__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }

// LDS traffic of one wavefront, ordered: what the lanes stored before is visible to whichever lane reads it next
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void col_norm_kernel(const int* __restrict__ p, const double* __restrict__ x, int64_t n,
                                                       double* __restrict__ norm) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double ss = 0.0;
    for (int e = p[j]; e < p[j + 1]; ++e) ss = add_rn(ss, mul_rn(x[e], x[e]));
    norm[j] = sqrt(ss);
}

__global__ __launch_bounds__(256) void tile_offsets_kernel(const int* __restrict__ tp, const int* __restrict__ ti, int64_t m,
                                                           int ntiles, int* __restrict__ ts) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)(ntiles + 1) * m) return;
    const int64_t t = idx / m, r = idx - t * m;
    const int64_t first = t * T;                // ntiles * T is past every column: the end of the row
    int lo = tp[r], hi = tp[r + 1];
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)ti[mid] < first) lo = mid + 1; else hi = mid;
    }
    ts[idx] = lo;
}

__global__ __launch_bounds__(NT) void cosine_tile_kernel(const int* __restrict__ yp, const int* __restrict__ yi,
                                                         const double* __restrict__ yx, const int* __restrict__ ts,
                                                         const int* __restrict__ ti, const double* __restrict__ tx,
                                                         const double* __restrict__ norm_x, const double* __restrict__ norm_y,
                                                         int64_t m, int64_t nx, int64_t ny, int ntiles, double* __restrict__ C) {
    __shared__ double acc[WAVES][T];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double* a = acc[w];
    const int64_t items = ny * ntiles, stride = (int64_t)gridDim.x * WAVES;
    // tile-major: the wavefronts in flight at one time read the same tile of X^T
    for (int64_t it = (int64_t)blockIdx.x * WAVES + w; it < items; it += stride) {
        const int t = (int)(it / ny);
        const int64_t j = it - (int64_t)t * ny;
        const int64_t i0 = (int64_t)t * T;
        const int tw = (int)(nx - i0 < T ? nx - i0 : T);
        for (int q = lane; q < tw; q += 64) a[q] = 0.0;
        wave_sync();
        const int* ts0 = ts + (int64_t)t * m;
        const int* ts1 = ts0 + m;
        const int e1 = yp[j + 1];
        for (int eb = yp[j]; eb < e1; eb += 64) {
            // 64 stored entries of y_j and their row segments, one per lane; then row after row, in storage order
            const int cnt = e1 - eb < 64 ? e1 - eb : 64;
            int s = 0, en = 0;
            double v = 0.0;
            if (lane < cnt) {
                const int r = yi[eb + lane];
                v = yx[eb + lane];
                s = ts0[r];
                en = ts1[r];
            }
            for (int k = 0; k < cnt; ++k) {
                const int sk = __shfl(s, k), ek = __shfl(en, k);
                const double vk = __shfl(v, k);
                for (int q = sk + lane; q < ek; q += 64) {
                    const int c = ti[q] - (int)i0;          // in [0, tw) by the construction of ts
                    a[c] = add_rn(a[c], mul_rn(vk, tx[q]));
                }
                wave_sync();
            }
        }
        const double nj = norm_y[j];
        double* out = C + j * nx + i0;
        for (int q = lane; q < tw; q += 64) {
            const double den = mul_rn(norm_x[i0 + q], nj);
            out[q] = den > 0.0 ? a[q] / den : 0.0;
        }
        wave_sync();
    }
}

// the 64 lane partials of a wavefront, added as a butterfly: every lane ends with the same value
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = add_rn(s, __shfl_xor(s, off));
    return s;
}

__global__ __launch_bounds__(DNT) void dense_stats_kernel(const double* __restrict__ W, const double* __restrict__ R, int64_t m,
                                                          int64_t nwc, int64_t nrc, int method, double* __restrict__ mean,
                                                          double* __restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * (DNT / 64) + (threadIdx.x >> 6);
    if (col >= nwc + nrc) return;
    const double* src = col < nwc ? W + col * m : R + (col - nwc) * m;
    double mu = 0.0;
    if (method == 1) {
        double s = 0.0;
        for (int64_t r = lane; r < m; r += 64) s = add_rn(s, src[r]);
        mu = wave_sum(s) / (double)m;
    }
    double ss = 0.0;
    for (int64_t r = lane; r < m; r += 64) {
        const double d = sub_rn(src[r], mu);
        ss = add_rn(ss, mul_rn(d, d));
    }
    ss = wave_sum(ss);
    if (lane == 0) {
        mean[col] = mu;
        norm[col] = sqrt(ss);
    }
}

// grid (nchunk, reps).  mean: reps * kx values of the stack, then ky of R.  partial: [rep][chunk][b][a]
__global__ __launch_bounds__(DNT) void dense_partial_kernel(const double* __restrict__ W, const double* __restrict__ R, int64_t m,
                                                            int kx, int ky, int64_t chunk, const double* __restrict__ mean,
                                                            int64_t reps, double* __restrict__ partial) {
    __shared__ double sW[DSB][DK];
    __shared__ double sR[DSB][DK];
    const int tid = threadIdx.x, ta = tid & 15, tb = tid >> 4;
    const int64_t rep = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = c0 + chunk < m ? c0 + chunk : m;
    const double* Wq = W + rep * m * kx;
    const double* muW = mean + rep * kx;
    const double* muR = mean + reps * kx;
    double acc[8][8];
#pragma unroll
    for (int pa = 0; pa < 8; ++pa)
#pragma unroll
        for (int pb = 0; pb < 8; ++pb) acc[pa][pb] = 0.0;
    for (int64_t r0 = c0; r0 < c1; r0 += DSB) {
        const int nrows = (int)(c1 - r0 < DSB ? c1 - r0 : DSB);
        for (int idx = tid; idx < DSB * kx; idx += DNT) {
            const int rr = idx % DSB, col = idx / DSB;
            if (rr < nrows) sW[rr][col] = sub_rn(Wq[(int64_t)col * m + r0 + rr], muW[col]);
        }
        for (int idx = tid; idx < DSB * ky; idx += DNT) {
            const int rr = idx % DSB, col = idx / DSB;
            if (rr < nrows) sR[rr][col] = sub_rn(R[(int64_t)col * m + r0 + rr], muR[col]);
        }
        __syncthreads();
        for (int r = 0; r < nrows; ++r) {
#pragma unroll
            for (int pa = 0; pa < 8; ++pa) {
                if (16 * pa >= kx) break;
                const double wv = sW[r][(ta + 16 * pa) & (DK - 1)];
#pragma unroll
                for (int pb = 0; pb < 8; ++pb) {
                    if (16 * pb >= ky) break;
                    acc[pa][pb] = add_rn(acc[pa][pb], mul_rn(wv, sR[r][(tb + 16 * pb) & (DK - 1)]));
                }
            }
        }
        __syncthreads();
    }
    double* out = partial + (rep * gridDim.x + blockIdx.x) * (int64_t)kx * ky;
#pragma unroll
    for (int pa = 0; pa < 8; ++pa)
#pragma unroll
        for (int pb = 0; pb < 8; ++pb) {
            const int a = ta + 16 * pa, b = tb + 16 * pb;
            if (a < kx && b < ky) out[(int64_t)b * kx + a] = acc[pa][pb];
        }
}

__global__ __launch_bounds__(DNT) void dense_final_kernel(const double* __restrict__ partial, int kx, int ky, int64_t reps,
                                                          int nchunk, const double* __restrict__ norm, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * DNT + threadIdx.x;
    const int64_t per = (int64_t)kx * ky;
    if (idx >= reps * per) return;
    const int64_t rep = idx / per, ab = idx - rep * per;
    const int b = (int)(ab / kx), a = (int)(ab - (int64_t)b * kx);
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s = add_rn(s, partial[(rep * nchunk + c) * per + ab]);
    const double den = mul_rn(norm[rep * kx + a], norm[reps * kx + b]);
    out[idx] = den > 0.0 ? s / den : 0.0;
}

}  // namespace rsim
