// kernels_svd_reg.hip.h -- device kernels of the L21 / angular / graph-regularised deflation SVD (ops_svd.hip: rcppml_gpu_svd_reg_ex,
// rcppml_gpu_svd_reg_dense_ex).  The reference's CPU rules (svd/deflation.hpp:191-292, applied at :734-742 and :779-787), per side
// and per iteration, on the freshly divided update x with nsq = dc |u_hat|^2 (v side) or dc |v|^2 (u side):
//   L21      L2_eff = L2 + L21 / |x| when |x| > 1e-10, |x| taken before any shrinkage; then L2_eff -> L1 -> nonneg -> upper bound
//   angular  x -= (angular / nsq) F (F' x), F the k stored factors of that side, F' x taken after the element chain; k = 0: nothing
//   graph    x -= (lambda / nsq) (L x), L as passed (rows from its device transpose), x after the angular step
// Each term needs a quantity of the whole vector that is only known after a grid-wide reduction, so a side with a term on runs a
// chain in place of its one epilogue (kernels_svd.hip.h: defl_v_kernel / defl_u_kernel):
//   head      the epilogue's divide (and, without L21, its element chain); writes nsq for the rest of the chain and the mid partials
//   shrink    L21 only: finalises |x|^2, runs the element chain with L2_eff
//   angular   finalises F' x, subtracts
//   graph     spmv_csr of L on x (kernels_svd.hip.h), then the subtract
// Every link rewrites x in place and ends in block partials; the last one writes the partials the next stage already expects
// ([V_k' v, sum v, |v|^2] on the n side, [|u_raw|^2, u_raw . u_cur] on the m side), so defl_u_kernel's normalisation of v and
// defl_finish_kernel run unchanged.  A link reads the partials of the one before and writes another buffer, never the one it reads.
// Reductions are two-stage in block order and there are no float atomics, as everywhere in kernels_svd.hip.h; every link honours
// idle(st, it) and returns on S_BRKV / S_BRKU, which leaves x as the breaking kernel wrote it (zeros on the v side).
#pragma once
#include "kernels_svd.hip.h"

namespace rsv {

// v-update head (n).  As defl_v_kernel in M_LOOP, except: shrink = 0 leaves the divided update unregularised (L21 follows), and
// nsq_out[0] = dc |u_hat|^2.  Partials [V_k' x (k), sum x, |x|^2] -> P.
template <class T>
__global__ __launch_bounds__(WG) void reg_v_head_kernel(const T* __restrict__ y, int n, const T* __restrict__ V, int k,
                                                        const T* __restrict__ d, const T* __restrict__ Pm, int nbm, int center, T l1, T l2,
                                                        int nonneg, T ub, T dc, int shrink, T* __restrict__ vraw, T* __restrict__ P,
                                                        T* __restrict__ nsq_out, int* st, int it) {
    if (idle(st, it)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    finalize(Pm, nbm, k + 2, h);
    const T c = center ? h[k] : T(0), usq = h[k + 1] * dc;
    const bool brk = !(usq > T(0));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (brk) st[S_BRKV] = 1;
        nsq_out[0] = usq;
    }
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)n - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long j = r0 + r;
        T s = y[j] - c;
        for (int q = 0; q < k; ++q) s -= V[(long)q * n + j] * (d[q] * h[q]);
        if (brk) s = T(0);
        else {
            s = s / usq;
            if (shrink) s = regularize(s, l1, l2, nonneg, ub, usq);
        }
        xs[r] = s;
        vraw[j] = s;
    }
    if (brk) return;
    __syncthreads();
    Cols<T> C;
    C.X = V; C.ld = n; C.nx = k; C.e[0] = nullptr; C.e[1] = vraw; C.ne = 2;
    block_partials(xs, vraw, r0, cnt, C, P);
}

// u-update head (m).  As defl_u_kernel in M_LOOP (it normalises v too), except: shrink = 0 leaves the divided update unregularised,
// nsq_out[0] = dc |v|^2, and the partials are the mid ones [U_k' x (k), |x|^2, x . u_cur] -> P.
template <class T>
__global__ __launch_bounds__(WG) void reg_u_head_kernel(const T* __restrict__ t, int m, const T* __restrict__ U, int k,
                                                        const T* __restrict__ d, const T* __restrict__ Pn, int nbn, const T* __restrict__ mu,
                                                        T l1, T l2, int nonneg, T ub, T dc, int shrink, const T* __restrict__ vraw,
                                                        T* __restrict__ v, int n, T* __restrict__ uraw, const T* __restrict__ ucur,
                                                        T* __restrict__ P, T* __restrict__ nsq_out, int* st, int it) {
    if (idle(st, it)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    if (st[S_BRKV]) {                                // u_hat was zero: v = 0 (vraw holds zeros), u stays
        for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j];
        return;
    }
    finalize(Pn, nbn, k + 2, h);
    const T sv = sqrt(h[k + 1]);
    if (!(sv > T(0))) {                              // sigma = 0 after the v-update -> break, v not normalised
        if (blockIdx.x == 0 && threadIdx.x == 0) st[S_BRKU] = 1;
        for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j];
        return;
    }
    const T inv = T(1) / sv;
    for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j] * inv;
    const T vsq = h[k + 1] * inv * inv * dc;
    if (blockIdx.x == 0 && threadIdx.x == 0) nsq_out[0] = vsq;
    const T sm = mu ? h[k] * inv : T(0);
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)m - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long i = r0 + r;
        T s = t[i] * inv - (mu ? mu[i] * sm : T(0));
        for (int q = 0; q < k; ++q) s -= U[(long)q * m + i] * (d[q] * (h[q] * inv));
        s = s / vsq;
        if (shrink) s = regularize(s, l1, l2, nonneg, ub, vsq);
        xs[r] = s;
        uraw[i] = s;
    }
    __syncthreads();
    Cols<T> C;
    C.X = U; C.ld = m; C.nx = k; C.e[0] = uraw; C.e[1] = ucur; C.ne = 2;
    block_partials(xs, uraw, r0, cnt, C, P);
}

// the words that end a side's chain: the v side stops on S_BRKV, the u side on either
__device__ inline bool reg_off(const int* st, int it, int uside) { return idle(st, it) || st[S_BRKV] || (uside && st[S_BRKU]); }

// L21 (deflation.hpp:200-213): |x|^2 = the finalised column sq of Pin (np columns), L2_eff = l2 + l21 / |x| above the 1e-10 guard,
// then the element chain on x in place.  Partials of the new x against Cout -> Pout.
template <class T>
__global__ __launch_bounds__(WG) void reg_shrink_kernel(T* __restrict__ x, long len, const T* __restrict__ Pin, int nb, int np, int sq,
                                                        const T* __restrict__ nsq_in, T l1, T l2, T l21, int nonneg, T ub, Cols<T> Cout,
                                                        T* __restrict__ Pout, const int* st, int it, int uside) {
    if (reg_off(st, it, uside)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    finalize(Pin, nb, np, h);
    const T nsq = nsq_in[0], xn = sqrt(h[sq]);
    const T l2e = xn > T(1e-10) ? l2 + l21 / xn : l2;
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const T s = regularize(x[r0 + r], l1, l2e, nonneg, ub, nsq);
        xs[r] = s;
        x[r0 + r] = s;
    }
    __syncthreads();
    block_partials(xs, x, r0, cnt, Cout, Pout);
}

// angular (deflation.hpp:256-267): h = F' x = the first k finalised columns of Pin; x -= (angular / nsq) (F h), F h summed in
// factor order.  Partials of the new x against Cout -> Pout.
template <class T>
__global__ __launch_bounds__(WG) void reg_angular_kernel(T* __restrict__ x, long len, const T* __restrict__ F, int k,
                                                         const T* __restrict__ Pin, int nb, int np, const T* __restrict__ nsq_in, T ang,
                                                         Cols<T> Cout, T* __restrict__ Pout, const int* st, int it, int uside) {
    if (reg_off(st, it, uside)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    finalize(Pin, nb, np, h);
    const T w = ang / nsq_in[0];
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long i = r0 + r;
        T f = 0;
        for (int q = 0; q < k; ++q) f += F[(long)q * len + i] * h[q];
        const T s = x[i] - w * f;
        xs[r] = s;
        x[i] = s;
    }
    __syncthreads();
    block_partials(xs, x, r0, cnt, Cout, Pout);
}

// graph (deflation.hpp:283-292): x -= (lambda / nsq) lx with lx = L x from spmv_csr.  Partials of the new x against Cout -> Pout.
template <class T>
__global__ __launch_bounds__(WG) void reg_graph_kernel(T* __restrict__ x, long len, const T* __restrict__ lx, const T* __restrict__ nsq_in,
                                                       T lam, Cols<T> Cout, T* __restrict__ Pout, const int* st, int it, int uside) {
    if (reg_off(st, it, uside)) return;
    __shared__ T xs[CH];
    const T w = lam / nsq_in[0];
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long i = r0 + r;
        const T s = x[i] - w * lx[i];
        xs[r] = s;
        x[i] = s;
    }
    __syncthreads();
    block_partials(xs, x, r0, cnt, Cout, Pout);
}

}  // namespace rsv
