// kernels_svd_krylov.hip.h -- device kernels of the constrained block SVD, Krylov-Seeded Projected Refinement (ops_svd.hip,
// Engine::kspr; the reference's svd/krylov.hpp:456-643 restated).
//
// The block factors live component-fastest: W as k x m, V as k x n (leading dimension k), so one row's k values are one contiguous
// read.  One half-update (W = proj(A V (V'V + ridge)^-1), or the same for V with A' and W) is three launches:
//   ks_half_kernel    one wavefront per output row (a CSR row for W, a CSC column for V); a lane is a component (two components
//                     for 64 < k <= 128; for k <= 32 the wavefront splits into 64 / kp lane groups that share the row's nonzeros):
//                     b = row . F, minus the centering term, w = G^-1 b with the fp64 inverse read from global memory (it stays in
//                     cache), then L1 / nonneg / upper bound.  Writes the unnormalised row and per-block partials of the column norms.
//   ks_finish_kernel  re-adds the norm partials in block order, sets d, normalises in place, and emits per-block partials of the next
//                     Gram (k x k), of the (weighted) column sums and -- W side -- of |W - W_prev|^2 and |W_prev|^2.
//   ks_small_kernel   one workgroup: reduces those partials in block order, writes the pass's dW and the stop word, adds the ridge
//                     and L2, factorises (Cholesky in LDS) and inverts.  Always fp64, in both precisions.
// Every partial buffer is fp64, accumulated with compensation (ks_kadd) and re-added in block order by its consumer; the block size is fixed, so the sums do not depend on
// the device and two runs are bitwise equal.  Later launches exit at once on the stop word (kernels_svd.hip.h, idle()).
#pragma once
#include "kernels_svd.hip.h"

namespace rsv {

constexpr int KS_KMAX = 128;
constexpr int KS_RPW = 16, KS_RB = NW * KS_RPW;      // half-update: rows per wavefront / per block
constexpr int KS_GR = 256, KS_GS = 32;               // finish: rows per block / per LDS sub-chunk
constexpr int KS_TD = 16;                            // finish: the Gram is tiled over 16 x 16 threads, TI x TI entries each
enum { KS_ERR = 5 };                                 // state word: 0, or 1 + 2 * pass + (1: V-update, 0: W-update) of a failed pivot

__host__ __device__ inline int ks_np(int k) { return k * k + k + 2; }   // a block's record: Gram, column sums, dW numerator, denominator

// Compensated (Kahan) accumulation: s += x with the running error in c.  The Gram, norm and dW sums are long chains of like-signed
// terms; a plain chain drifts by several ulp, which shows in d as a common factor.
__device__ inline void ks_kadd(double& s, double& c, double x) {
    const double y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

template <class T> __device__ inline T ks_project(T v, T ns, T l1, int nonneg, T ub) {   // krylov.hpp:162-204 with L2 = 0
    if (!(ns > T(0))) return T(0);
    if (l1 > T(0)) {
        const T th = l1 / (T(2) * ns);
        v = v > th ? v - th : (v < -th ? v + th : T(0));
    }
    if (nonneg) v = v > T(0) ? v : T(0);
    if (ub > T(0)) v = v < ub ? v : ub;
    return v;
}

// p / idx / x: the compressed rows of the output side (CSR of A for W, CSC of A for V); F: the fixed factor (k x other side);
// center: 0 none, 1 W side (b -= mu[row] cs), 2 V side (b -= cs); cs: 1'V or mu'W from the previous small kernel.
template <class T>
__global__ __launch_bounds__(WG) void ks_half_kernel(const int* __restrict__ p, const int* __restrict__ idx, const T* __restrict__ x,
                                                     long len, const T* __restrict__ F, int k, int kp, const double* __restrict__ Ginv,
                                                     const double* __restrict__ nsq, const double* __restrict__ cs,
                                                     const T* __restrict__ mu, int center, T l1, int nonneg, T ub,
                                                     T* __restrict__ Xraw, double* __restrict__ Pn, const int* st, int it) {
    if (idle(st, it)) return;
    __shared__ double red[NW][KS_KMAX];
    const int w = threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    const int c0 = l % kp, g = l / kp, ng = WAVE / kp, c1 = c0 + WAVE;
    const bool on0 = c0 < k, on1 = c1 < k;              // c1 only when k > 64 (then kp = 64, one group)
    const T ns0 = on0 ? (T)nsq[c0] : T(0), ns1 = on1 ? (T)nsq[c1] : T(0);
    const double s0 = center && on0 ? cs[c0] : 0.0, s1 = center && on1 ? cs[c1] : 0.0;
    double q0 = 0, q1 = 0, e0 = 0, e1 = 0;
    for (int r = 0; r < KS_RPW; ++r) {
        const long row = (long)blockIdx.x * KS_RB + (long)w * KS_RPW + r;
        if (row >= len) break;
        T a0 = 0, a1 = 0;
        for (int e = p[row] + g; e < p[row + 1]; e += ng) {
            const T xv = x[e];
            const T* f = F + (long)idx[e] * k;
            if (on0) a0 += xv * f[c0];
            if (on1) a1 += xv * f[c1];
        }
        for (int o = kp; o < WAVE; o <<= 1) a0 += __shfl_xor(a0, o);
        if (center == 1) { a0 -= mu[row] * (T)s0; a1 -= mu[row] * (T)s1; }
        else if (center == 2) { a0 -= (T)s0; a1 -= (T)s1; }
        const double b0 = (double)a0, b1 = (double)a1;
        double w0 = 0, w1 = 0;
        for (int j = 0; j < k; ++j) {
            const double bj = j < WAVE ? __shfl(b0, j) : __shfl(b1, j - WAVE);
            const double* gr = Ginv + (long)j * k;
            if (on0) w0 += gr[c0] * bj;
            if (on1) w1 += gr[c1] * bj;
        }
        const T v0 = ks_project((T)w0, ns0, l1, nonneg, ub), v1 = ks_project((T)w1, ns1, l1, nonneg, ub);
        if (g == 0) {
            if (on0) { Xraw[row * k + c0] = v0; ks_kadd(q0, e0, (double)v0 * (double)v0); }
            if (on1) { Xraw[row * k + c1] = v1; ks_kadd(q1, e1, (double)v1 * (double)v1); }
        }
    }
    if (g == 0) {
        if (on0) red[w][c0] = q0;
        if (on1) red[w][c1] = q1;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < k; c += WG) {
        double s = 0;
        for (int q = 0; q < NW; ++q) s += red[q][c];
        Pn[(long)blockIdx.x * k + c] = s;
    }
}

// X (k x len): raw = 1: d = |column| from the partials Pn (nbh blocks) when above eps100, else 0; X /= d where d > 0 (in place), d ->
// d_out.  Then the block's record into PG: X'X, the column sums weighted by wt (nullptr: ones), and with Xold the two dW sums.
// TI: ceil(k / 16) rounded up to 1, 2, 4 or 8.
template <class T, int TI>
__global__ __launch_bounds__(WG) void ks_finish_kernel(T* __restrict__ X, long len, int k, const double* __restrict__ Pn, int nbh,
                                                       T eps100, int raw, const T* __restrict__ wt, const T* __restrict__ Xold,
                                                       T* __restrict__ d_out, double* __restrict__ PG, const int* st, int it) {
    if (idle(st, it)) return;
    __shared__ T xs[KS_GS * KS_KMAX];
    __shared__ T ds[KS_KMAX];
    __shared__ double red[NW];
    if (raw) {
        for (int c = threadIdx.x; c < k; c += WG) {
            double s = 0, sc = 0;
            for (int b = 0; b < nbh; ++b) ks_kadd(s, sc, Pn[(long)b * k + c]);
            const T nrm = (T)sqrt(s);
            const T d = nrm > eps100 ? nrm : T(0);
            ds[c] = d;
            if (blockIdx.x == 0) d_out[c] = d;
        }
        __syncthreads();
    }
    const int kk = k * k;
    const int ta = threadIdx.x / KS_TD, tb = threadIdx.x % KS_TD;
    double acc[TI][TI], cmp[TI][TI];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) acc[i][j] = cmp[i][j] = 0;
    double csum = 0, csc = 0, num = 0, nmc = 0, den = 0, dnc = 0;
    const long b0 = (long)blockIdx.x * KS_GR;
    const long bend = min(len, b0 + KS_GR);
    for (long r0 = b0; r0 < bend; r0 += KS_GS) {
        const int cnt = (int)min((long)KS_GS, bend - r0);
        for (int e = threadIdx.x; e < cnt * k; e += WG) {
            const long ge = r0 * k + e;
            T v = X[ge];
            if (raw) {
                const T d = ds[e % k];
                if (d > T(0)) { v /= d; X[ge] = v; }
            }
            xs[e] = v;
            if (Xold) {
                const double o = (double)Xold[ge], df = (double)v - o;
                ks_kadd(num, nmc, df * df);
                ks_kadd(den, dnc, o * o);
            }
        }
        __syncthreads();
        if (threadIdx.x < k)
            for (int r = 0; r < cnt; ++r) ks_kadd(csum, csc, (double)xs[r * k + threadIdx.x] * (wt ? (double)wt[r0 + r] : 1.0));
        for (int r = 0; r < cnt; ++r) {
            double av[TI], bv[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int a = ta + KS_TD * i, b = tb + KS_TD * i;
                av[i] = a < k ? (double)xs[r * k + a] : 0.0;
                bv[i] = b < k ? (double)xs[r * k + b] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TI; ++j) ks_kadd(acc[i][j], cmp[i][j], av[i] * bv[j]);
        }
        __syncthreads();
    }
    double* rec = PG + (long)blockIdx.x * ks_np(k);
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TI; ++j) {
            const int a = ta + KS_TD * i, b = tb + KS_TD * j;
            if (a < k && b < k) rec[a * k + b] = acc[i][j];
        }
    if (threadIdx.x < k) rec[kk + threadIdx.x] = csum;
    num = block_sum(num, red);
    den = block_sum(den, red);
    if (threadIdx.x == 0) { rec[kk + k] = num; rec[kk + k + 1] = den; }
}

// One workgroup.  side 0: after the W-update of pass `it` (factorises W'W for its V-update, and from the second pass on writes
// dW = |W - W_prev| / (|W_prev| + eps) and, below tol, the stop word: pass `it` still finishes); side 1: after the V-update (records
// it + 1 passes done and, unless the loop ends here, factorises V'V for the W-update of pass it + 1; it = -1: the seed).
// Outputs: Ginv = (G + ridge I)^-1, nsq = diag(G) before the ridge, cs = the column sums.  Li: k x k scratch.
// A non-positive (or NaN) pivot stops the loop before the update it would feed and leaves its code in st[KS_ERR].
__global__ __launch_bounds__(WG) void ks_small_kernel(const double* __restrict__ PG, int nb, int k, double ridge,
                                                      double* __restrict__ Ginv, double* __restrict__ Li, double* __restrict__ nsq,
                                                      double* __restrict__ cs, double* __restrict__ dw_out, double tol, double eps,
                                                      int* st, int it, int side, int last) {
    if (idle(st, it)) return;
    __shared__ double G[KS_KMAX * KS_KMAX];
    __shared__ double ex[2];
    const int kk = k * k, np = ks_np(k);
    const bool ends = side == 1 && (last || st[S_STOP] <= it + 1);
    for (int e = threadIdx.x; e < np; e += WG) {
        double s = 0, sc = 0;
        for (int b = 0; b < nb; ++b) ks_kadd(s, sc, PG[(long)b * np + e]);
        if (e < kk) G[e] = s;
        else if (e < kk + k) cs[e - kk] = s;
        else ex[e - kk - k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (side == 1) st[S_ITERS] = it + 1;
        else if (it > 0) {
            const double dw = sqrt(ex[0]) / (sqrt(ex[1]) + eps);
            dw_out[it - 1] = dw;
            if (dw < tol) st[S_STOP] = it + 1;
        }
    }
    if (ends) return;
    for (int c = threadIdx.x; c < k; c += WG) {
        nsq[c] = G[c * k + c];
        G[c * k + c] += ridge;
    }
    // Cholesky, lower triangle in place
    for (int j = 0; j < k; ++j) {
        __syncthreads();
        const double piv = G[j * k + j];
        if (!(piv > 0.0)) {
            if (threadIdx.x == 0) {
                const int feeds = side == 0 ? it : it + 1;
                st[KS_ERR] = 1 + 2 * feeds + (side == 0 ? 1 : 0);
                st[S_STOP] = feeds;
            }
            return;
        }
        const double ljj = sqrt(piv);
        __syncthreads();
        if (threadIdx.x == 0) G[j * k + j] = ljj;
        for (int i = j + 1 + threadIdx.x; i < k; i += WG) G[i * k + j] /= ljj;
        __syncthreads();
        const int r = k - j - 1;
        for (int e = threadIdx.x; e < r * r; e += WG) {
            const int i = j + 1 + e / r, c = j + 1 + e % r;
            if (c <= i) G[i * k + c] -= G[i * k + j] * G[c * k + j];
        }
    }
    __syncthreads();
    // Li = L^-1 (lower), one column per thread by forward substitution
    for (int j = threadIdx.x; j < k; j += WG) {
        for (int i = 0; i < j; ++i) Li[i * k + j] = 0.0;
        Li[j * k + j] = 1.0 / G[j * k + j];
        for (int i = j + 1; i < k; ++i) {
            double s = 0;
            for (int c = j; c < i; ++c) s += G[i * k + c] * Li[c * k + j];
            Li[i * k + j] = -s / G[i * k + i];
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kk; e += WG) G[e] = Li[e];
    __syncthreads();
    // G^-1 = Li' Li
    for (int e = threadIdx.x; e < kk; e += WG) {
        const int a = e / k, b = e % k;
        double s = 0;
        for (int i = max(a, b); i < k; ++i) s += G[i * k + a] * G[i * k + b];
        Ginv[e] = s;
    }
}

}  // namespace rsv
