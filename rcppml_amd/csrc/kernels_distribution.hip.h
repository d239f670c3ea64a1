// kernels_distribution.hip.h -- device side of the distribution diagnostics (ops_distribution.hip): the reference's
// score_test_distribution / diagnose_zero_inflation / diagnose_dispersion (R/auto_distribution.R:194-452) without the dense m x n
// product R builds on the host.  fp64 throughout.
//
//   mu_tile_kernel<MODE>   mu = (W diag(d)) H a 64 x 64 tile at a time (an FMA chain over k from LDS panels), never written; epilogues:
//                          ZI    per-tile row / column partials of exp(-max(mu, 1e-8)) (+ zero counts of dense x)
//                          SCORE per-block partials of sum(r^2 / mu'^p - 1) per power, sum((r^2 - mu') / mu'^2), non-integral count
//                          DISP  phi = (x - mu')^2 / mu'^p into the one m x n buffer (sparse input: x = 0 here)
//   nz_kernel<MODE>        the per-nonzero gather of loss_nonzeros_kernel (rk::wave_pred) with the SCORE epilogue over x != 0, or
//                          the DISP overwrite of the stored entries (one wavefront per column, rows strictly increasing: race-free)
//   seg_trim_kernel<G>     trimmed means by exact radix selection of the lo-th and hi-th keys of each segment (a column: G = 1,
//                          contiguous; 16 rows: G = 16, stride m), then one summing pass; glob_* the same over all m*n values
//
// Every floating-point sum has a fixed order (per-thread chains, then fixed trees, then block partials added in block order).
// Integer counts use integer atomics.  All indices into m x n arrays are 64-bit.
#pragma once
#include "kernels.hip.h"

namespace rdist {

constexpr int TM = 64, TN = 64, KC = 16, NT = 256;
constexpr int MAXP = 8;                 // powers per score test
enum { MODE_ZI = 0, MODE_SCORE = 1, MODE_DISP = 2 };

struct MuArgs {
    const double* A;                    // k x m: a(f, i) = W_T(f, i) d_f (formed on the host, as R's W %*% diag(d))
    const double* H;                    // k x n
    const double* X;                    // dense x, column-major m x n; NULL for sparse input
    int64_t m, n;
    int k, ntr;                         // ntr = row tiles
    int npow;
    double pw[MAXP];
    double min_mu, power;
    double* part;                       // SCORE: (npow + 1) partials per block
    unsigned long long* nonint;         // SCORE: count of non-integral x
    double* prow;                       // ZI: ntc x m row partials
    double* pcol;                       // ZI: ntr x n column partials
    unsigned long long* zrow;           // ZI, dense: observed zeros per row / column
    unsigned long long* zcol;
    double* phi;                        // DISP: m x n, column-major
};

// R's `^`: x * x for p = 2, 1 for p = 0, pow otherwise
__device__ __forceinline__ double rpow(double x, double p) { return p == 2.0 ? x * x : (p == 0.0 ? 1.0 : pow(x, p)); }

template <int MODE>
__global__ __launch_bounds__(NT) void mu_tile_kernel(MuArgs a) {
    __shared__ double sA[KC][TM + 1];
    __shared__ double sH[KC][TN + 1];
    __shared__ double red[16][TM + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int tr = (int)(blockIdx.x % (unsigned)a.ntr), tc = (int)(blockIdx.x / (unsigned)a.ntr);
    const int64_t r0 = (int64_t)tr * TM, c0 = (int64_t)tc * TN;
    double acc[4][4];
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
    // entry (i, j) of this thread: row r0 + tx + 16 i, column c0 + ty + 16 j
    if (MODE == MODE_DISP) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t gj = c0 + ty + 16 * j;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t gi = r0 + tx + 16 * i;
                if (gi < a.m && gj < a.n) {
                    const double mu = fmax(acc[i][j], a.min_mu);
                    const double x = a.X ? a.X[gj * a.m + gi] : 0.0;
                    const double r = x - mu;
                    a.phi[gj * a.m + gi] = (r * r) / rpow(mu, a.power);
                }
            }
        }
    } else if (MODE == MODE_ZI) {
        double e[4][4];
        float z[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t gi = r0 + tx + 16 * i, gj = c0 + ty + 16 * j;
                const bool ok = gi < a.m && gj < a.n;
                e[i][j] = ok ? exp(-fmax(acc[i][j], 1e-8)) : 0.0;
                z[i][j] = (ok && a.X && a.X[gj * a.m + gi] == 0.0) ? 1.f : 0.f;
            }
        // row partials: this thread's 4 columns, then the 16 column groups in order
#pragma unroll
        for (int i = 0; i < 4; ++i) red[ty][tx + 16 * i] = ((e[i][0] + e[i][1]) + e[i][2]) + e[i][3];
        __syncthreads();
        if (t < TM && r0 + t < a.m) {
            double s = 0.0;
            for (int g = 0; g < 16; ++g) s += red[g][t];
            a.prow[(int64_t)tc * a.m + r0 + t] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) red[tx][ty + 16 * j] = ((e[0][j] + e[1][j]) + e[2][j]) + e[3][j];
        __syncthreads();
        if (t < TN && c0 + t < a.n) {
            double s = 0.0;
            for (int g = 0; g < 16; ++g) s += red[g][t];
            a.pcol[(int64_t)tr * a.n + c0 + t] = s;
        }
        if (a.X) {            // zero counts (exact small integers in double)
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) red[ty][tx + 16 * i] = ((z[i][0] + z[i][1]) + z[i][2]) + z[i][3];
            __syncthreads();
            if (t < TM && r0 + t < a.m) {
                double s = 0.0;
                for (int g = 0; g < 16; ++g) s += red[g][t];
                if (s > 0) atomicAdd(&a.zrow[r0 + t], (unsigned long long)s);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) red[tx][ty + 16 * j] = ((z[0][j] + z[1][j]) + z[2][j]) + z[3][j];
            __syncthreads();
            if (t < TN && c0 + t < a.n) {
                double s = 0.0;
                for (int g = 0; g < 16; ++g) s += red[g][t];
                if (s > 0) atomicAdd(&a.zcol[c0 + t], (unsigned long long)s);
            }
        }
    } else {   // MODE_SCORE (dense x)
        double s[MAXP + 1];
#pragma unroll
        for (int q = 0; q <= MAXP; ++q) s[q] = 0.0;
        int bad = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t gi = r0 + tx + 16 * i, gj = c0 + ty + 16 * j;
                if (gi < a.m && gj < a.n) {
                    const double x = a.X[gj * a.m + gi];
                    const double mu = fmax(acc[i][j], a.min_mu);
                    const double r = x - mu, r2 = r * r;
#pragma unroll
                    for (int q = 0; q < MAXP; ++q)
                        if (q < a.npow) s[q] += r2 / rpow(mu, a.pw[q]) - 1.0;
                    s[MAXP] += (r2 - mu) / (mu * mu);
                    bad += x != rint(x);
                }
            }
        __shared__ double sh[4];
        double* out = a.part + (int64_t)blockIdx.x * (a.npow + 1);
#pragma unroll
        for (int q = 0; q < MAXP; ++q)
            if (q < a.npow) {
                const double v = rk::block_sum_256(s[q], sh);
                if (t == 0) out[q] = v;
            }
        const double v = rk::block_sum_256(s[MAXP], sh);
        if (t == 0) out[a.npow] = v;
        const int nb = __syncthreads_count(bad > 0);
        if (nb > 0) {
            const int mine = bad;
            if (mine) atomicAdd(a.nonint, (unsigned long long)mine);
        }
    }
}

// One wavefront per column over its stored entries; p from rk::wave_pred (the gather of loss_nonzeros_kernel).
//   MODE_SCORE: entries with x != 0 -- partials as mu_tile_kernel's, the count of such entries and of non-integral ones
//   MODE_DISP:  phi(row, j) of every stored entry (the all-entries pass wrote the x = 0 value there)
template <int MODE>
__global__ __launch_bounds__(NT) void nz_kernel(const int* __restrict__ colptr, const int* __restrict__ rowidx,
                                                const double* __restrict__ vals, const double* __restrict__ W_T,
                                                const double* __restrict__ d, const double* __restrict__ Hm, MuArgs a,
                                                unsigned long long* __restrict__ count) {
    __shared__ double sh[4][MAXP + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    double s[MAXP + 1];
#pragma unroll
    for (int q = 0; q <= MAXP; ++q) s[q] = 0.0;
    unsigned long long cnt = 0, bad = 0;
    if (j < a.n) {
        for (int e = colptr[j]; e < colptr[j + 1]; ++e) {
            const int row = rowidx[e];
            const double x = vals[e];
            if (MODE == MODE_SCORE && x == 0.0) continue;     // which(data != 0)
            const double pd = rk::wave_pred(W_T, d, Hm, row, j, a.k, lane);
            const double mu = fmax(pd, a.min_mu);
            const double r = x - mu, r2 = r * r;
            if (MODE == MODE_DISP) {
                if (lane == 0) a.phi[j * a.m + row] = r2 / rpow(mu, a.power);
            } else {
#pragma unroll
                for (int q = 0; q < MAXP; ++q)
                    if (q < a.npow) s[q] += r2 / rpow(mu, a.pw[q]) - 1.0;
                s[MAXP] += (r2 - mu) / (mu * mu);
                ++cnt;
                bad += x != rint(x);
            }
        }
    }
    if (MODE == MODE_SCORE) {
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q <= MAXP; ++q) sh[wave][q] = s[q];
            if (cnt) atomicAdd(count, cnt);
            if (bad) atomicAdd(a.nonint, bad);
        }
        __syncthreads();
        double* out = a.part + (int64_t)blockIdx.x * (a.npow + 1);
        if (threadIdx.x < a.npow) {
            const int q = threadIdx.x;
            out[q] = ((sh[0][q] + sh[1][q]) + sh[2][q]) + sh[3][q];
        } else if (threadIdx.x == a.npow) {
            out[a.npow] = ((sh[0][MAXP] + sh[1][MAXP]) + sh[2][MAXP]) + sh[3][MAXP];
        }
    }
}

// out[q] = sum over blocks b (in order) of part[b * width + q], q < width; one workgroup.
__global__ __launch_bounds__(NT) void sum_block_partials(const double* __restrict__ part, int64_t nblk, int width,
                                                         double* __restrict__ out) {
    __shared__ double sh[4];
    for (int q = 0; q < width; ++q) {
        double acc = 0.0;
        for (int64_t b = threadIdx.x; b < nblk; b += NT) acc += part[b * width + q];
        const double v = rk::block_sum_256(acc, sh);
        if (threadIdx.x == 0) out[q] = v;
    }
}

// out[i] = sum over p (in order) of part[p * len + i]
__global__ __launch_bounds__(NT) void sum_strided_partials(const double* __restrict__ part, int64_t nparts, int64_t len,
                                                           double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= len) return;
    double s = 0.0;
    for (int64_t p = 0; p < nparts; ++p) s += part[p * len + i];
    out[i] = s;
}

// ---------------------------------------------------------------------------------------------------------- trimmed means
// phi >= 0 (or +inf), so its IEEE bits order like its value.  Ranks are 1-based: the trimmed mean is the mean of the order
// statistics lo..hi.  With klo / khi the keys of ranks lo / hi, cle = #(key <= klo), clt = #(key < khi):
//   klo == khi: every value in lo..hi equals it;  otherwise
//   sum = sum(klo < key < khi) + (cle - lo + 1) * v(klo) + (hi - clt) * v(khi)   over hi - lo + 1 values.
__device__ __forceinline__ double trim_result(double between, long long cle, long long clt, unsigned long long klo,
                                              unsigned long long khi, long long lo, long long hi) {
    const double vlo = __longlong_as_double((long long)klo), vhi = __longlong_as_double((long long)khi);
    if (klo == khi) return vlo;
    return (between + (double)(cle - lo + 1) * vlo + (double)(hi - clt) * vhi) / (double)(hi - lo + 1);
}

__device__ __forceinline__ unsigned long long phi_key(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned long long prefix_mask(int shift) { return shift >= 56 ? 0ull : (~0ull << (shift + 8)); }

// G segments per workgroup; segment s = blockIdx.x * G + g holds phi[s * sstride + e * estride], e < N.
template <int G>
__global__ __launch_bounds__(NT) void seg_trim_kernel(const double* __restrict__ phi, int64_t nseg, int64_t sstride,
                                                      int64_t estride, int64_t N, long long lo, long long hi,
                                                      double* __restrict__ out) {
    __shared__ unsigned int hist[G][2][256];
    __shared__ unsigned long long pre[G][2];
    __shared__ long long rank[G][2];
    __shared__ double ssum[NT];
    __shared__ long long scle[NT], sclt[NT];
    constexpr int STEP = NT / G;
    const int t = threadIdx.x, g = t % G;
    const int64_t s = (int64_t)blockIdx.x * G + g;
    const bool valid = s < nseg;
    const double* base = phi + (valid ? s : 0) * sstride;
    if (t < 2 * G) { pre[t >> 1][t & 1] = 0ull; rank[t >> 1][t & 1] = (t & 1) ? hi : lo; }
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int q = t; q < G * 512; q += NT) (&hist[0][0][0])[q] = 0u;
        __syncthreads();
        const unsigned long long msk = prefix_mask(shift), p0 = pre[g][0], p1 = pre[g][1];
        if (valid)
            for (int64_t e = t / G; e < N; e += STEP) {
                const unsigned long long key = phi_key(base[e * estride]);
                const unsigned dg = (unsigned)(key >> shift) & 255u;
                if ((key & msk) == p0) atomicAdd(&hist[g][0][dg], 1u);
                if ((key & msk) == p1) atomicAdd(&hist[g][1][dg], 1u);
            }
        __syncthreads();
        if (t < 2 * G) {
            const int gg = t >> 1, q = t & 1;
            long long cum = 0;
            const long long want = rank[gg][q];
            for (int dg = 0; dg < 256; ++dg) {
                const long long c = hist[gg][q][dg];
                if (cum + c >= want) {
                    pre[gg][q] |= (unsigned long long)dg << shift;
                    rank[gg][q] = want - cum;
                    break;
                }
                cum += c;
            }
        }
        __syncthreads();
    }
    const unsigned long long klo = pre[g][0], khi = pre[g][1];
    double between = 0.0;
    long long cle = 0, clt = 0;
    if (valid)
        for (int64_t e = t / G; e < N; e += STEP) {
            const double v = base[e * estride];
            const unsigned long long key = phi_key(v);
            if (key > klo && key < khi) between += v;
            cle += key <= klo;
            clt += key < khi;
        }
    ssum[t] = between; scle[t] = cle; sclt[t] = clt;
    __syncthreads();
    if (t < G && valid) {
        double b = 0.0;
        long long a1 = 0, a2 = 0;
        for (int u = t; u < NT; u += G) { b += ssum[u]; a1 += scle[u]; a2 += sclt[u]; }
        out[s] = trim_result(b, a1, a2, klo, khi, lo, hi);
    }
}

// Global selection: state of the two searches in device memory, one histogram pass per digit over the whole array.
struct GSel {
    unsigned long long pre[2];
    long long rank[2];
};

__global__ __launch_bounds__(NT) void glob_hist_kernel(const double* __restrict__ phi, int64_t N, int shift,
                                                       const GSel* __restrict__ st, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int h[2][256];
    for (int q = threadIdx.x; q < 512; q += NT) (&h[0][0])[q] = 0u;
    __syncthreads();
    const unsigned long long msk = prefix_mask(shift), p0 = st->pre[0], p1 = st->pre[1];
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < N; e += (int64_t)gridDim.x * NT) {
        const unsigned long long key = phi_key(phi[e]);
        const unsigned dg = (unsigned)(key >> shift) & 255u;
        if ((key & msk) == p0) atomicAdd(&h[0][dg], 1u);
        if ((key & msk) == p1) atomicAdd(&h[1][dg], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 512; q += NT) {
        const unsigned c = (&h[0][0])[q];
        if (c) atomicAdd(&hist[q], (unsigned long long)c);
    }
}

__global__ void glob_choose_kernel(GSel* __restrict__ st, unsigned long long* __restrict__ hist, int shift) {
    const int t = threadIdx.x;
    if (t < 2) {
        long long cum = 0;
        const long long want = st->rank[t];
        for (int dg = 0; dg < 256; ++dg) {
            const long long c = (long long)hist[t * 256 + dg];
            if (cum + c >= want) {
                st->pre[t] |= (unsigned long long)dg << shift;
                st->rank[t] = want - cum;
                break;
            }
            cum += c;
        }
    }
    __syncthreads();
    for (int q = t; q < 512; q += blockDim.x) hist[q] = 0ull;
}

// per-block partials: sum of the values strictly between the keys, #(key <= klo), #(key < khi)
__global__ __launch_bounds__(NT) void glob_sum_kernel(const double* __restrict__ phi, int64_t N, const GSel* __restrict__ st,
                                                      double* __restrict__ psum, long long* __restrict__ pcnt) {
    __shared__ double sh[4];
    __shared__ long long c1[NT], c2[NT];
    const unsigned long long klo = st->pre[0], khi = st->pre[1];
    double between = 0.0;
    long long cle = 0, clt = 0;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < N; e += (int64_t)gridDim.x * NT) {
        const double v = phi[e];
        const unsigned long long key = phi_key(v);
        if (key > klo && key < khi) between += v;
        cle += key <= klo;
        clt += key < khi;
    }
    const double b = rk::block_sum_256(between, sh);
    c1[threadIdx.x] = cle; c2[threadIdx.x] = clt;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a1 = 0, a2 = 0;
        for (int u = 0; u < NT; ++u) { a1 += c1[u]; a2 += c2[u]; }
        psum[blockIdx.x] = b;
        pcnt[2 * blockIdx.x] = a1;
        pcnt[2 * blockIdx.x + 1] = a2;
    }
}

__global__ __launch_bounds__(NT) void glob_final_kernel(const double* __restrict__ psum, const long long* __restrict__ pcnt, int nblk,
                                                        const GSel* __restrict__ st, long long lo, long long hi, double* __restrict__ out) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += NT) acc += psum[b];
    const double v = rk::block_sum_256(acc, sh);
    if (threadIdx.x == 0) {
        long long a1 = 0, a2 = 0;
        for (int b = 0; b < nblk; ++b) { a1 += pcnt[2 * b]; a2 += pcnt[2 * b + 1]; }
        out[0] = trim_result(v, a1, a2, st->pre[0], st->pre[1], lo, hi);
    }
}

}  // namespace rdist
