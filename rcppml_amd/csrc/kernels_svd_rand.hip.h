// kernels_svd_rand.hip.h -- device kernels of the randomized block SVD (ops_svd.hip, Engine::randomized; the reference's
// Halko-Martinsson-Tropp method, svd/randomized.hpp:59-241, restated).
//
// The blocks live component-fastest as in KSPR: l x m and l x n with leading dimension l = k + oversampling (l <= 128), so one
// output row's l values are one contiguous read.  The kernels of a fit:
//   rs_omega_kernel   the sketch Omega(i, j) = uniform<T>() - 0.5 of SplitMix64 draw j n + i, a pure function of the index.
//   rs_prod_kernel    Y = A~ X from the CSR or Z = A~' X from the CSC: one wavefront per output row, a lane is a component (two
//                     components for 64 < l <= 128; for l <= 32 the wavefront splits into 64 / lp lane groups that share the row's
//                     nonzeros).  The centering term is - mu_row (1'X) or - (mu'X), with the l-vector re-added from the records
//                     of the block it multiplies.
//   rs_chol_kernel    one workgroup: re-adds the Gram records in block order, factorises G = R'R in LDS and writes R^-1.  A pivot
//                     that is not above thr times its column's original diagonal (or is NaN) is rejected: that column of R^-1 is
//                     zero, the column of Q becomes zero, and the factorisation goes on.  Always fp64.
//   rs_apply_kernel   X <- X R^-1 in place, one wavefront per row.
//   rs_rotate_kernel  out (rows x k, column-major) = X W for a small l x k matrix W.
// Every kernel that writes a block also writes, per workgroup of RS_RB rows, a record of that block: its l x l Gram and its l
// column sums (weighted by wt, or plain), fp64 with compensated accumulation.  The consumers re-add the records in block order and
// RS_RB is fixed, so the sums do not depend on the device and two runs are bitwise equal.  No atomics.
#pragma once
#include "kernels_svd_krylov.hip.h"

namespace rsv {

constexpr int RS_LMAX = 128;
constexpr int RS_RPW = 4, RS_RB = NW * RS_RPW;       // rows per wavefront / per workgroup, and the rows of one record
constexpr int RS_GS = RS_RB;                         // record: rows per LDS sub-chunk

__host__ __device__ inline int rs_np(int l) { return l * l + l; }   // a record: Gram, column sums

// sum over b < nb of P[b * stride] in block order, compensated.  The loads go out sixteen at a time: one at a time this chain is
// pure memory latency, and it sits at the head of every consumer.
__device__ inline double rs_readd(const double* __restrict__ P, int nb, long stride) {
    double s = 0, sc = 0;
    int b = 0;
    for (; b + 16 <= nb; b += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = P[(long)(b + u) * stride];
#pragma unroll
        for (int u = 0; u < 16; ++u) ks_kadd(s, sc, v[u]);
    }
    for (; b < nb; ++b) ks_kadd(s, sc, P[(long)b * stride]);
    return s;
}

// The record of rows [b0, bend) of X (l x len), written by this workgroup before the call (the caller synchronises).
// TI: ceil(l / 16) rounded up to 1, 2, 4 or 8.  gram = 0: the column sums only.  At TI = 8 the Gram's 8 x 8 entries per thread and
// their compensation terms would not fit the register file, so the rows are staged twice and each pass keeps a 4 x 8 half.
template <class T, int TI>
__device__ void rs_record(const T* X, long b0, long bend, int l, const T* __restrict__ wt, int gram, double* __restrict__ rec, T* xs) {
    constexpr int NH = TI > 4 ? 2 : 1, HI = TI / NH;
    const int ta = threadIdx.x / KS_TD, tb = threadIdx.x % KS_TD;
    for (int h = 0; h < (gram ? NH : 1); ++h) {
        double acc[HI][TI], cmp[HI][TI];
#pragma unroll
        for (int i = 0; i < HI; ++i)
#pragma unroll
            for (int j = 0; j < TI; ++j) acc[i][j] = cmp[i][j] = 0;
        double csum = 0, csc = 0;
        for (long r0 = b0; r0 < bend; r0 += RS_GS) {
            const int cnt = (int)min((long)RS_GS, bend - r0);
            for (int e = threadIdx.x; e < cnt * l; e += WG) xs[e] = X[r0 * l + e];
            __syncthreads();
            if (h == 0 && threadIdx.x < l)
                for (int r = 0; r < cnt; ++r) ks_kadd(csum, csc, (double)xs[r * l + threadIdx.x] * (wt ? (double)wt[r0 + r] : 1.0));
            if (gram)
                for (int r = 0; r < cnt; ++r) {
                    double av[HI], bv[TI];
#pragma unroll
                    for (int i = 0; i < HI; ++i) {
                        const int a = ta + KS_TD * (h * HI + i);
                        av[i] = a < l ? (double)xs[r * l + a] : 0.0;
                    }
#pragma unroll
                    for (int j = 0; j < TI; ++j) {
                        const int b = tb + KS_TD * j;
                        bv[j] = b < l ? (double)xs[r * l + b] : 0.0;
                    }
#pragma unroll
                    for (int i = 0; i < HI; ++i)
#pragma unroll
                        for (int j = 0; j < TI; ++j) ks_kadd(acc[i][j], cmp[i][j], av[i] * bv[j]);
                }
            __syncthreads();
        }
        if (gram) {
#pragma unroll
            for (int i = 0; i < HI; ++i)
#pragma unroll
                for (int j = 0; j < TI; ++j) {
                    const int a = ta + KS_TD * (h * HI + i), b = tb + KS_TD * j;
                    if (a < l && b < l) rec[a * l + b] = acc[i][j];
                }
        }
        if (h == 0 && threadIdx.x < l) rec[l * l + threadIdx.x] = csum;
    }
}

// X (l x n) = Omega': element (i, j) is draw j n + i of the stream of `seed` (rng/rng.hpp:89-104, :213-219), minus 0.5.
template <class T, int TI>
__global__ __launch_bounds__(WG) void rs_omega_kernel(T* X, long n, int l, unsigned long long seed, double* __restrict__ Pout) {
    __shared__ T xs[RS_GS * RS_LMAX];
    const long b0 = (long)blockIdx.x * RS_RB, bend = min(n, b0 + RS_RB);
    const int cnt = (int)(bend - b0);
    for (int e = threadIdx.x; e < cnt * l; e += WG) {
        const long i = b0 + e / l;
        const int j = e % l;
        unsigned long long z = seed + ((unsigned long long)j * (unsigned long long)n + (unsigned long long)i + 1ull) * 0x9e3779b97f4a7c15ull;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z = z ^ (z >> 31);
        X[i * l + j] = static_cast<T>(z) / static_cast<T>(UINT64_MAX) - T(0.5);
    }
    __syncthreads();
    rs_record<T, TI>(X, b0, bend, l, nullptr, 0, Pout + (long)blockIdx.x * rs_np(l), xs);
}

// p / idx / x: the compressed rows of the output side (CSR of A for Y, CSC of A for Z); F: the block it multiplies (l x other
// side) and Pin its nbin records (read for the column sums when centred); center: 0 none, 1 Y side (- mu[row] cs), 2 Z side (- cs).
template <class T, int TI>
__global__ __launch_bounds__(WG) void rs_prod_kernel(const int* __restrict__ p, const int* __restrict__ idx, const T* __restrict__ x,
                                                     long len, const T* __restrict__ F, int l, int lp, const double* __restrict__ Pin,
                                                     int nbin, const T* __restrict__ mu, int center, T* X, double* __restrict__ Pout) {
    __shared__ T xs[RS_GS * RS_LMAX];
    __shared__ double cs[RS_LMAX];
    if (center) {
        const int np = rs_np(l);
        for (int c = threadIdx.x; c < l; c += WG) cs[c] = rs_readd(Pin + l * l + c, nbin, np);
        __syncthreads();
    }
    const int w = threadIdx.x / WAVE, ln = threadIdx.x % WAVE;
    const int c0 = ln % lp, g = ln / lp, ng = WAVE / lp, c1 = c0 + WAVE;
    const bool on0 = c0 < l, on1 = c1 < l;              // c1 only when l > 64 (then lp = 64, one group)
    const T s0 = center && on0 ? (T)cs[c0] : T(0), s1 = center && on1 ? (T)cs[c1] : T(0);
    const long b0 = (long)blockIdx.x * RS_RB, bend = min(len, b0 + RS_RB);
    for (int r = 0; r < RS_RPW; ++r) {
        const long row = b0 + (long)w * RS_RPW + r;
        if (row >= len) break;
        T a0 = 0, a1 = 0;
        // the row's nonzeros 64 at a time: one coalesced load of indices and values, then lane group g takes entries g, g + ng, ...
        // by shuffle, so the gathers of F do not wait on a load of idx (the order of each lane's sum is the entries' order)
        const int pe = p[row + 1];
        for (int e0 = p[row]; e0 < pe; e0 += WAVE) {
            const int cnt = min(WAVE, pe - e0);
            const int iv = ln < cnt ? idx[e0 + ln] : 0;
            const T xl = ln < cnt ? x[e0 + ln] : T(0);
#pragma unroll 4
            for (int t = 0; t < cnt; t += ng) {
                const int src = min(t + g, WAVE - 1);
                const int col = __shfl(iv, src);
                const T xv = __shfl(xl, src);
                if (t + g < cnt) {
                    const T* f = F + (long)col * l;
                    if (on0) a0 += xv * f[c0];
                    if (on1) a1 += xv * f[c1];
                }
            }
        }
        for (int o = lp; o < WAVE; o <<= 1) a0 += __shfl_xor(a0, o);
        if (center == 1) { a0 -= mu[row] * s0; a1 -= mu[row] * s1; }
        else if (center == 2) { a0 -= s0; a1 -= s1; }
        if (g == 0) {
            if (on0) X[row * l + c0] = a0;
            if (on1) X[row * l + c1] = a1;
        }
    }
    __syncthreads();
    rs_record<T, TI>(X, b0, bend, l, nullptr, 1, Pout + (long)blockIdx.x * rs_np(l), xs);
}

// One workgroup.  G = the records' Grams re-added in block order.  final: G -> Gout and nothing else.  Else the Cholesky factor
// L = R' of G in LDS, a pivot accepted only above thr * (its original diagonal), and Rinv[b * l + a] = R^-1(b, a); a rejected
// pivot leaves row and column of R^-1 zero.  Li: l x l scratch.
__global__ __launch_bounds__(WG) void rs_chol_kernel(const double* __restrict__ P, int nb, int l, double thr, double* __restrict__ Rinv,
                                                     double* __restrict__ Li, double* __restrict__ Gout, int final) {
    __shared__ double G[RS_LMAX * RS_LMAX];
    __shared__ double d0[RS_LMAX];
    __shared__ int dead[RS_LMAX];
    const int ll = l * l, np = rs_np(l);
    for (int e = threadIdx.x; e < ll; e += WG) {
        const double s = rs_readd(P + e, nb, np);
        if (final) Gout[e] = s;
        else G[e] = s;
    }
    if (final) return;
    __syncthreads();
    for (int c = threadIdx.x; c < l; c += WG) { d0[c] = G[c * l + c]; dead[c] = 0; }
    for (int j = 0; j < l; ++j) {
        __syncthreads();
        const double piv = G[j * l + j];
        const bool ok = piv > thr * d0[j];                  // false for a NaN pivot too
        __syncthreads();
        if (!ok) {
            if (threadIdx.x == 0) dead[j] = 1;
            for (int i = j + 1 + threadIdx.x; i < l; i += WG) G[i * l + j] = 0.0;
            continue;
        }
        const double ljj = sqrt(piv);
        if (threadIdx.x == 0) G[j * l + j] = ljj;
        for (int i = j + 1 + threadIdx.x; i < l; i += WG) G[i * l + j] /= ljj;
        __syncthreads();
        const int r = l - j - 1;
        for (int e = threadIdx.x; e < r * r; e += WG) {
            const int i = j + 1 + e / r, c = j + 1 + e % r;
            if (c <= i) G[i * l + c] -= G[i * l + j] * G[c * l + j];
        }
    }
    __syncthreads();
    // Li = L^-1 (lower), one column per thread by forward substitution; a dead index has a zero row and a zero column
    for (int j = threadIdx.x; j < l; j += WG) {
        for (int i = 0; i < j; ++i) Li[i * l + j] = 0.0;
        Li[j * l + j] = dead[j] ? 0.0 : 1.0 / G[j * l + j];
        for (int i = j + 1; i < l; ++i) {
            double s = 0;
            if (!dead[i] && !dead[j]) {
                for (int c = j; c < i; ++c) s += G[i * l + c] * Li[c * l + j];
                s = -s / G[i * l + i];
            }
            Li[i * l + j] = s;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ll; e += WG) Rinv[e] = Li[(e % l) * l + e / l];
}

// X (l x len) <- X R^-1 in place (row x: q_a = sum_b R^-1(b, a) x_b, accumulated in fp64), then the block's record.
template <class T, int TI>
__global__ __launch_bounds__(WG) void rs_apply_kernel(T* X, long len, int l, const double* __restrict__ Rinv, const T* __restrict__ wt,
                                                      int gram, double* __restrict__ Pout) {
    __shared__ T xs[RS_GS * RS_LMAX];
    const int w = threadIdx.x / WAVE, c0 = threadIdx.x % WAVE, c1 = c0 + WAVE;
    const bool on0 = c0 < l, on1 = c1 < l;
    const long b0 = (long)blockIdx.x * RS_RB, bend = min(len, b0 + RS_RB);
    for (int r = 0; r < RS_RPW; ++r) {
        const long row = b0 + (long)w * RS_RPW + r;
        if (row >= len) break;
        const double x0 = on0 ? (double)X[row * l + c0] : 0.0, x1 = on1 ? (double)X[row * l + c1] : 0.0;
        double q0 = 0, q1 = 0;
        for (int b = 0; b < l; ++b) {
            const double xb = b < WAVE ? __shfl(x0, b) : __shfl(x1, b - WAVE);
            const double* rr = Rinv + (long)b * l;
            if (on0) q0 += rr[c0] * xb;
            if (on1) q1 += rr[c1] * xb;
        }
        if (on0) X[row * l + c0] = (T)q0;
        if (on1) X[row * l + c1] = (T)q1;
    }
    __syncthreads();
    rs_record<T, TI>(X, b0, bend, l, wt, gram, Pout + (long)blockIdx.x * rs_np(l), xs);
}

// out (len x k, column-major) = X' W: X is l x len, W is l x k with W[b * k + c] (fp64); one wavefront per row of out
template <class T>
__global__ __launch_bounds__(WG) void rs_rotate_kernel(const T* __restrict__ X, long len, int l, const double* __restrict__ W, int k,
                                                       T* __restrict__ out) {
    const int c0 = threadIdx.x % WAVE, c1 = c0 + WAVE;
    const long row = (long)blockIdx.x * NW + threadIdx.x / WAVE;
    if (row >= len) return;
    const double x0 = c0 < l ? (double)X[row * l + c0] : 0.0, x1 = c1 < l ? (double)X[row * l + c1] : 0.0;
    double q0 = 0, q1 = 0;
    for (int b = 0; b < l; ++b) {
        const double xb = b < WAVE ? __shfl(x0, b) : __shfl(x1, b - WAVE);
        const double* wr = W + (long)b * k;
        if (c0 < k) q0 += wr[c0] * xb;
        if (c1 < k) q1 += wr[c1] * xb;
    }
    if (c0 < k) out[(long)c0 * len + row] = (T)q0;
    if (c1 < k) out[(long)c1 * len + row] = (T)q1;
}

}  // namespace rsv
