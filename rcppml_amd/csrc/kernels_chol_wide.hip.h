// ============================================================================
// kernels_chol_wide.hip.h -- Cholesky + clip for the ranks the lane-per-column solve cannot hold: 64 < k <= 256 in fp64 and
// 128 < k <= 256 in fp32 (kernels.hip.h: chol_factor_kernel keeps the whole Gram in LDS, chol_solve_kernel keeps x[KP] in one
// lane's registers).  Same contract: x = L^-T L^-1 (b - l1); x = max(x, 0) if nonneg; x = min(x, ub) if ub > 0.
//
// Blocks are BS x BS with BS = 16 (fp64, v_mfma_f64_16x16x4_f64) or 32 (fp32, v_mfma_f32_32x32x2_f32); the Gram is padded with
// identity to KP = nb * BS.  Workspace (global, WS_CHOL): W (KP x KP, column-major: the trailing matrix, then L below the
// diagonal blocks), LT (the same L row-major), invD and invDT (nb blocks: inv(L_ii) and its transpose, column-major).
//
// chol_wide_factor_kernel -- ONE workgroup of four wavefronts, right-looking by panels of BS columns:
//   1. the panel (rows j0.., BS columns) goes to LDS;
//   2. wave 0 factorises the diagonal block unblocked IN REGISTERS (lane = row, readlane broadcasts of the pivot column; the
//      non-positive-pivot guard |d| + 1e-30 of chol_factor_kernel) and inverts it by triangular substitution (lane = column of
//      the inverse);
//   3. every thread takes one row below the block and substitutes it against L11^T (L11 is an LDS broadcast);
//   4. the trailing update A22 -= L21 L21^T runs on MFMA, one lower block per wave round-robin, both operands read from the
//      LDS panel, the accumulator loaded from and stored to W.
//
// chol_wide_solve_kernel -- a blocked TRSM as a GEMM chain.  One wavefront owns BS columns and keeps their whole KP x BS
// solution in MFMA accumulators (nb blocks; 128 VGPRs at k = 256 in either type).  Forward, block row i:
//   X_i += (-L_ip) X_p for p < i, then X_i = inv(L_ii) X_i; backward the same with L^T.  No division, no serial chain in a block.
// The four waves of a workgroup share each block row of L (negated while staged) and its inverse block through LDS, double
// buffered: one barrier per block row.
// THE CRUX -- a solved block sits in accumulator layout and is the multiplicand of every later step.  Neither a transposed
// system nor an LDS round trip is needed: with X as the B operand (K x N), the lane that holds D(row, col) in accumulator
// register v is the lane that must supply B(K-slot, col) of an MFMA step, provided the K-slots of step v are ENUMERATED as the
// rows register v holds:  fp64: row(v) = (lane >> 4) + 4 v,  fp32: row(v) = (v & 3) + 8 (v >> 2) + 4 (lane >> 5).
// A sum over K does not care about the order of its terms, so step v takes x[p][v] as its B operand as it stands and the A
// operand (L from LDS, [column][row]: conflict-free) is read at column row(v).  The solved block never leaves its registers.
// Column tails (ncols % BS) and rank tails (k % BS) are masked on load and store; the result of a column does not depend on
// the grid.  No atomics.
// ============================================================================
#pragma once
#include "kernels.hip.h"

namespace rk {

template <class T> struct CholWide;
template <> struct CholWide<double> {
    static constexpr int BS = 16, NV = 4;      // block size; accumulator registers per lane = MFMA steps per block product
    typedef f64x4 Acc;
    static __device__ __forceinline__ int row(int v, int lane) { return (lane >> 4) + 4 * v; }
    static __device__ __forceinline__ Acc mfma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ double bcast(double x, int l) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
    }
};
template <> struct CholWide<float> {
    static constexpr int BS = 32, NV = 16;
    typedef f32x16 Acc;
    static __device__ __forceinline__ int row(int v, int lane) { return (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5); }
    static __device__ __forceinline__ Acc mfma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float bcast(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
};

constexpr int CHOLW_THREADS = 256, CHOLW_WAVES = 4, CHOLW_KMAX = 256;

template <class T>
__global__ __launch_bounds__(CHOLW_THREADS) void chol_wide_factor_kernel(const T* __restrict__ G, int k, int nb, T* __restrict__ W,
                                                                          T* __restrict__ LT, T* __restrict__ invD, T* __restrict__ invDT) {
    typedef CholWide<T> M;
    typedef typename M::Acc Acc;
    constexpr int BS = M::BS, NV = M::NV;
    __shared__ T P[CHOLW_KMAX * BS];          // the panel, P(r, c) at [c * h + r], h = rows left
    __shared__ T dinv[BS];                    // 1 / L11(c, c)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KP = nb * BS;
    for (int e = tid; e < KP * KP; e += CHOLW_THREADS) {
        const int i = e % KP, j = e / KP;
        W[e] = (i < k && j < k) ? G[(int64_t)j * k + i] : (i == j ? T(1) : T(0));
    }
    __syncthreads();
    for (int jb = 0; jb < nb; ++jb) {
        const int j0 = jb * BS, h = KP - j0;
        for (int e = tid; e < h * BS; e += CHOLW_THREADS) P[e] = W[(int64_t)(j0 + e / h) * KP + j0 + e % h];
        __syncthreads();
        if (wave == 0) {
            // lane r holds row r of the diagonal block (lanes >= BS repeat a row and write nothing)
            const int r = lane & (BS - 1);
            T a[BS], il[BS];
#pragma unroll
            for (int c = 0; c < BS; ++c) a[c] = P[c * h + r];
#pragma unroll
            for (int c = 0; c < BS; ++c) {
                T d = M::bcast(a[c], c);
                if (!(d > T(0))) d = tabs(d) + T(1e-30);
                const T l = sqrt(d);
                il[c] = T(1) / l;
                a[c] = r == c ? l : a[c] / l;
#pragma unroll
                for (int c2 = c + 1; c2 < BS; ++c2) a[c2] = tfma(-a[c], M::bcast(a[c], c2), a[c2]);
            }
            // lane c solves L z = e_c: column c of inv(L11)
            T z[BS];
#pragma unroll
            for (int i = 0; i < BS; ++i) {
                T s = r == i ? T(1) : T(0);
#pragma unroll
                for (int p = 0; p < i; ++p) s = tfma(-M::bcast(a[p], i), z[p], s);
                z[i] = s * il[i];
            }
            if (lane < BS) {
                T* Zb = invD + (size_t)jb * BS * BS;
                T* ZTb = invDT + (size_t)jb * BS * BS;
#pragma unroll
                for (int c = 0; c < BS; ++c) {
                    const T lv = r >= c ? a[c] : T(0);
                    P[c * h + r] = lv;
                    W[(int64_t)(j0 + c) * KP + j0 + r] = lv;
                    LT[(int64_t)(j0 + r) * KP + j0 + c] = lv;
                    if (r == c) dinv[c] = il[c];
                    Zb[r * BS + c] = z[c];             // z[c] on lane r is Z(c, r)
                    ZTb[c * BS + r] = z[c];
                }
            }
        }
        __syncthreads();
        // rows below the diagonal block: x L11^T = a, one row per thread
        for (int r = BS + tid; r < h; r += CHOLW_THREADS) {
            T x[BS];
#pragma unroll
            for (int c = 0; c < BS; ++c) x[c] = P[c * h + r];
#pragma unroll
            for (int c = 0; c < BS; ++c) {
                T s = x[c];
#pragma unroll
                for (int q = 0; q < c; ++q) s = tfma(-x[q], P[q * h + c], s);
                x[c] = s * dinv[c];
            }
#pragma unroll
            for (int c = 0; c < BS; ++c) {
                P[c * h + r] = x[c];
                W[(int64_t)(j0 + c) * KP + j0 + r] = x[c];
                LT[(int64_t)(j0 + r) * KP + j0 + c] = x[c];
            }
        }
        __syncthreads();
        // A22 -= L21 L21^T on the lower blocks (diagonal blocks whole), one block per wave in turn
        const int nt = nb - jb - 1, cc = lane & (BS - 1);
        int t = 0;
        for (int bj = 0; bj < nt; ++bj)
            for (int bi = bj; bi < nt; ++bi, ++t) {
                if ((t & (CHOLW_WAVES - 1)) != wave) continue;
                T* Wb = W + (int64_t)(j0 + BS + bj * BS + cc) * KP + j0 + BS + bi * BS;
                Acc acc;
#pragma unroll
                for (int v = 0; v < NV; ++v) acc[v] = Wb[M::row(v, lane)];
#pragma unroll
                for (int s = 0; s < NV; ++s) {
                    const T* Pq = P + M::row(s, lane) * h + BS + cc;
                    acc = M::mfma(-Pq[bi * BS], Pq[bj * BS], acc);
                }
#pragma unroll
                for (int v = 0; v < NV; ++v) Wb[M::row(v, lane)] = acc[v];
            }
        __syncthreads();
    }
}

// the negated block row i of L (columns below i * BS) and inv(L_ii) behind it, as [column][row]
template <class T>
__device__ __forceinline__ void chol_wide_stage_fwd(T* d, const T* __restrict__ W, const T* __restrict__ invD, int i, int KP, int tid) {
    constexpr int BS = CholWide<T>::BS;
    const int n = i * BS * BS;
    for (int e = tid; e < n; e += CHOLW_THREADS) d[e] = -W[(int64_t)(e / BS) * KP + i * BS + e % BS];
    for (int e = tid; e < BS * BS; e += CHOLW_THREADS) d[n + e] = invD[(size_t)n + e];
}
// the negated block column i of L below block i, transposed (read from the row-major copy), and inv(L_ii)^T in slot i
template <class T>
__device__ __forceinline__ void chol_wide_stage_bwd(T* d, const T* __restrict__ LT, const T* __restrict__ invDT, int i, int KP, int tid) {
    constexpr int BS = CholWide<T>::BS;
    const int n = i * BS * BS, lo = (i + 1) * BS * BS, hi = KP * BS;
    for (int e = lo + tid; e < hi; e += CHOLW_THREADS) d[e] = -LT[(int64_t)(e / BS) * KP + i * BS + e % BS];
    for (int e = tid; e < BS * BS; e += CHOLW_THREADS) d[n + e] = invDT[(size_t)n + e];
}

template <class T, int NBMAX>
__global__ __launch_bounds__(CHOLW_THREADS) void chol_wide_solve_kernel(const T* __restrict__ W, const T* __restrict__ LT,
                                                                         const T* __restrict__ invD, const T* __restrict__ invDT,
                                                                         const T* __restrict__ B, T* __restrict__ X, int k, int nb,
                                                                         int64_t ncols, T l1_pre, int nonneg, T ub_post) {
    typedef CholWide<T> M;
    typedef typename M::Acc Acc;
    constexpr int BS = M::BS, NV = M::NV, BB = BS * BS;
    __shared__ T Ls[2][NBMAX * BB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cc = lane & (BS - 1);
    const int KP = nb * BS;
    const int64_t j = ((int64_t)blockIdx.x * CHOLW_WAVES + wave) * BS + cc;
    const bool jok = j < ncols;                       // a wave past the last column solves zeros and stores nothing
    const T* bj = B + (jok ? j : 0) * (int64_t)k;
    Acc x[NBMAX];
#pragma unroll
    for (int b = 0; b < NBMAX; ++b)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int r = b * BS + M::row(v, lane);
            x[b][v] = (jok && r < k) ? bj[r] - l1_pre : T(0);
        }
    chol_wide_stage_fwd<T>(Ls[0], W, invD, 0, KP, tid);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NBMAX; ++i) {
        if (i < nb) {
            if (i + 1 < nb) chol_wide_stage_fwd<T>(Ls[(i + 1) & 1], W, invD, i + 1, KP, tid);
            else chol_wide_stage_bwd<T>(Ls[(i + 1) & 1], LT, invDT, i, KP, tid);
            const T* d = Ls[i & 1] + cc;
#pragma unroll
            for (int p = 0; p < i; ++p)
#pragma unroll
                for (int s = 0; s < NV; ++s) x[i] = M::mfma(d[p * BB + M::row(s, lane) * BS], x[p][s], x[i]);
            Acc tacc;
#pragma unroll
            for (int v = 0; v < NV; ++v) tacc[v] = T(0);
#pragma unroll
            for (int s = 0; s < NV; ++s) tacc = M::mfma(d[i * BB + M::row(s, lane) * BS], x[i][s], tacc);
            x[i] = tacc;
            __syncthreads();
        }
    }
    // block row i of the backward pass is staged in buffer (i + 1) & 1
#pragma unroll
    for (int i = NBMAX - 1; i >= 0; --i) {
        if (i < nb) {
            if (i > 0) chol_wide_stage_bwd<T>(Ls[i & 1], LT, invDT, i - 1, KP, tid);
            const T* d = Ls[(i + 1) & 1] + cc;
#pragma unroll
            for (int p = i + 1; p < NBMAX; ++p)
                if (p < nb) {
#pragma unroll
                    for (int s = 0; s < NV; ++s) x[i] = M::mfma(d[p * BB + M::row(s, lane) * BS], x[p][s], x[i]);
                }
            Acc tacc;
#pragma unroll
            for (int v = 0; v < NV; ++v) tacc[v] = T(0);
#pragma unroll
            for (int s = 0; s < NV; ++s) tacc = M::mfma(d[i * BB + M::row(s, lane) * BS], x[i][s], tacc);
            x[i] = tacc;
            if (i > 0) __syncthreads();
        }
    }
    if (!jok) return;
    T* xj = X + j * (int64_t)k;
#pragma unroll
    for (int b = 0; b < NBMAX; ++b)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int r = b * BS + M::row(v, lane);
            if (r < k) {
                T val = x[b][v];
                if (nonneg) val = val > T(0) ? val : T(0);
                if (ub_post > T(0)) val = val < ub_post ? val : ub_post;
                xj[r] = val;
            }
        }
}

}  // namespace rk
