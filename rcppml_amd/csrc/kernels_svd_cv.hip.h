// kernels_svd_cv.hip.h -- device kernels of the cross-validated / masked deflation SVD (ops_svd.hip: rcppml_gpu_svd_cv_ex,
// rcppml_gpu_svd_cv_dense_ex), beside kernels_svd.hip.h.
//
// The hold-out rule is the reference's CPU rule (nmf/speckled_cv.hpp LazySpeckledMask::is_holdout -> rng/rng.hpp:129-170):
// entry (i, j) is held out when cv_hash_dev(seed, i, j) < UINT64_MAX / inv_prob; threshold = 0 holds nothing out (no CV).  The
// obs-mask is a pattern CSC with ascending rows, asked by bisection (cv_user_masked).
//   train_values   the training matrix: the values of A with held-out and obs-masked entries set to 0, same pattern
//                  (svd/test_entries.hpp:264-315, svd/deflation.hpp:452-487); per-column counts of obs-masked entries
//   test_entries   the held-out entries (row, column, value - row mean) in column-major order (svd/test_entries.hpp:84-141):
//                  a count pass (rows == nullptr) writes per-column counts, the host scans them, the write pass places each entry
//                  at offset[column] + entries of earlier steps + its rank in the step's ballot.  Nothing is ordered by arrival,
//                  so two runs give the same arrays.
//   test_loss      r_e -= sigma u[row_e] v[col_e] in place, and the block partials of r^2 (svd/test_entries.hpp:43-65); the
//                  host re-adds them in block order.
// One wavefront walks one column, 64 entries (sparse) or 64 rows (dense) per step; no float atomics anywhere.
#pragma once
#include "kernels_cv.hip.h"
#include "kernels_svd.hip.h"

namespace rsv {

// entries of the step's ballot below lane l
__device__ inline int ballot_rank(unsigned long long bal, int l) { return __popcll(bal & ((1ull << l) - 1ull)); }

// sparse (ri != nullptr): x holds the values in CSC order; dense: x is the column-major m x n matrix and p is not read
template <class T>
__global__ __launch_bounds__(WG) void train_values(const int* __restrict__ p, const int* __restrict__ ri, const T* __restrict__ x,
                                                   int m, int n, unsigned long long seed, unsigned long long threshold,
                                                   const int* __restrict__ mp, const int* __restrict__ mi, T* __restrict__ xt,
                                                   int* __restrict__ n_masked) {
    const int j = blockIdx.x * NW + threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    if (j >= n) return;
    const long lo = ri ? p[j] : (long)j * m, hi = ri ? p[j + 1] : (long)(j + 1) * m;
    int masked = 0;
    for (long b = lo; b < hi; b += WAVE) {
        const long e = b + l;
        const bool on = e < hi;
        const int i = on ? (ri ? ri[e] : (int)(e - lo)) : 0;
        const bool um = on && rk::cv_user_masked(mp, mi, j, i);
        const bool held = on && rk::cv_hash_dev(seed, (unsigned)i, (unsigned)j) < threshold;
        if (on) xt[e] = (um || held) ? T(0) : x[e];
        masked += __popcll(__ballot(um));
    }
    if (l == 0 && n_masked) n_masked[j] = masked;
}

// count pass: rows == nullptr, cnt[j] = held-out entries of column j.  write pass: off = exclusive scan of cnt.
template <class T>
__global__ __launch_bounds__(WG) void test_entries(const int* __restrict__ p, const int* __restrict__ ri, const T* __restrict__ x,
                                                   int m, int n, unsigned long long seed, unsigned long long threshold,
                                                   const T* __restrict__ mu, const int* __restrict__ off, int* __restrict__ cnt,
                                                   int* __restrict__ rows, int* __restrict__ cols, T* __restrict__ res) {
    const int j = blockIdx.x * NW + threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    if (j >= n) return;
    const long lo = ri ? p[j] : (long)j * m, hi = ri ? p[j + 1] : (long)(j + 1) * m;
    int seen = 0;
    for (long b = lo; b < hi; b += WAVE) {
        const long e = b + l;
        const bool on = e < hi;
        const int i = on ? (ri ? ri[e] : (int)(e - lo)) : 0;
        const bool held = on && rk::cv_hash_dev(seed, (unsigned)i, (unsigned)j) < threshold;
        const unsigned long long bal = __ballot(held);
        if (rows && held) {
            const long at = (long)off[j] + seen + ballot_rank(bal, l);
            rows[at] = i;
            cols[at] = j;
            res[at] = x[e] - (mu ? mu[i] : T(0));
        }
        seen += __popcll(bal);
    }
    if (!rows && l == 0) cnt[j] = seen;
}

// residual update and the partials of sum r^2: P[blockIdx.x]
template <class T>
__global__ __launch_bounds__(WG) void test_loss(const int* __restrict__ rows, const int* __restrict__ cols, T* __restrict__ res,
                                                long count, const T* __restrict__ u, const T* __restrict__ v, T sigma,
                                                T* __restrict__ P) {
    __shared__ T xs[CH];
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, count - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long e = r0 + r;
        const T d = res[e] - sigma * u[rows[e]] * v[cols[e]];
        res[e] = d;
        xs[r] = d;
    }
    __syncthreads();
    Cols<T> C;
    C.e[0] = res; C.ne = 1;
    block_partials(xs, res, r0, cnt, C, P);
}

}  // namespace rsv
