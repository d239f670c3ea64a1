// ============================================================================
// kernels_cv.hip.h -- cross-validation half-update for the MSE loss and the held-out error, k <= 64 (k > 64:
// kernels_wide.hip.h; IRLS losses: kernels_cv_irls.hip.h).
//
// Reference nmf/fit_cv.hpp:420-478 / :591-830, nmf/cv_detail.hpp:66-85,304-405, nmf/speckled_cv.hpp: speckled holdout mask
// defined by SplitMix64::hash(seed, i, j) < UINT64_MAX / inv_prob (rng/rng.hpp:129-170), no mask matrix.  One wavefront per
// column j of D (D = A on the H side, A^T with transposed = 1 on the W side; the mask is always asked in the coordinates of A):
//   b       = sum over the column's TRAIN nonzeros  a F(row, :)
//   G_local = G - sum over the column's TEST rows  F(row, :) F(row, :)^T   (mask_zeros: held-out nonzeros only;
//             otherwise every held-out row, zeros included -- the 64 lanes hash 64 rows at a time)
//   x       = cholesky_clip(G_local, b - L1) or CD(G_local, b, x; L1 inside, cd_maxit sweeps, no tolerance), started from
//             the current column without a warm-start correction of b, exactly as the reference does.
// ============================================================================
#pragma once
#include "mfma_gram_tile.hip.h"

namespace rk {

__device__ __forceinline__ unsigned long long cv_hash_dev(unsigned long long seed, unsigned i, unsigned j) {
    unsigned long long h = seed + (unsigned long long)i * 0x9e3779b97f4a7c15ULL + (unsigned long long)j * 0x6c62272e07bb0142ULL;
    h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ULL;
    h = (h ^ (h >> 27)) * 0x94d049bb133111ebULL;
    return h ^ (h >> 31);
}
// is entry `row` of column `col` of the walked matrix (A, or A^T with transposed = 1) held out?
__device__ __forceinline__ bool cv_held(unsigned long long seed, int transposed, unsigned col, unsigned row, unsigned long long threshold) {
    return (transposed ? cv_hash_dev(seed, col, row) : cv_hash_dev(seed, row, col)) < threshold;
}

// user mask of a CV fit (fit_cv.hpp:327-331; cv_detail.hpp:408-415 is_user_masked_h): pattern CSC in the orientation of the CSC the
// kernel walks, rows ascending inside a column; NULL = none.  Bisection: masks are sparse and the question is asked per entry.
__device__ __forceinline__ bool cv_user_masked(const int* __restrict__ mp, const int* __restrict__ mi, int64_t j, int row) {
    if (!mp) return false;
    int lo = mp[j];
    const int end = mp[j + 1];
    int hi = end;
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (mi[mid] < row) lo = mid + 1; else hi = mid; }
    return lo < end && mi[lo] == row;
}
// is `row` one of the stored rows of column [ts, te) of a CSC with ascending rows?
__device__ __forceinline__ bool cv_row_stored(const int* __restrict__ rowidx, int ts, int te, int row) {
    int lo = ts, hi = te;
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (rowidx[mid] < row) lo = mid + 1; else hi = mid; }
    return lo < te && rowidx[lo] == row;
}

// (mp, mi: optional user mask, cv_detail.hpp:433-505 -- a masked row that is not already a test row leaves b and joins the rows of
// the Gram correction, whether its entry is a nonzero or not)
template <class T, int KP>   // KP in {32, 64}
__global__ __launch_bounds__(256) void cv_solve_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const T* __restrict__ vals, int64_t ncols, int nrows,
    const T* __restrict__ F, const T* __restrict__ Gfull, T* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, T l1, int nonneg, int maxit, int solver_mode,
    const int* __restrict__ mp = nullptr, const int* __restrict__ mi = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* Gl = reinterpret_cast<T*>(smem_raw) + (size_t)wave * KP * KP;   // [c][r]
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const bool fok = lane < k;
    const int ll = lane < KP ? lane : 0;
    wave_gram_load<T, KP>(Gl, Gfull, k, lane);
    const unsigned col = (unsigned)j;
    // train right-hand side (and, with mask_zeros, the Gram correction of the held-out nonzeros)
    T b = T(0);
    for (int t = colptr[j]; t < colptr[j + 1]; ++t) {
        const int row = rowidx[t];
        const bool held = cv_held(seed, transposed, col, (unsigned)row, threshold);
        const T fr = fok ? F[(int64_t)row * k + lane] : T(0);
        if (!held) {
            if (!cv_user_masked(mp, mi, j, row)) b = tfma(vals[t], fr, b);
        } else if (mask_zeros) {
            wave_gram_downdate<T, KP>(Gl, fr, k, lane);
        }
    }
    if (!mask_zeros) {      // every held-out row of this column, zeros included
        for (int r0 = 0; r0 < nrows; r0 += 64) {
            const int r = r0 + lane;
            const bool held = r < nrows && cv_held(seed, transposed, col, (unsigned)r, threshold);
            unsigned long long m = __ballot(held);
            while (m) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                const int row = r0 + bit;
                const T fr = fok ? F[(int64_t)row * k + lane] : T(0);
                wave_gram_downdate<T, KP>(Gl, fr, k, lane);
            }
        }
    }
    if (mp) {               // user-masked rows that are not test rows: out of the Gram as well
        const int ts = colptr[j], te = colptr[j + 1];
        for (int t = mp[j]; t < mp[j + 1]; ++t) {
            const int row = mi[t];
            const bool held = cv_held(seed, transposed, col, (unsigned)row, threshold);
            if (held && (!mask_zeros || cv_row_stored(rowidx, ts, te, row))) continue;      // already corrected above
            const T fr = fok ? F[(int64_t)row * k + lane] : T(0);
            wave_gram_downdate<T, KP>(Gl, fr, k, lane);
        }
    }
    RK_WAVE_SYNC();
    T x = fok ? X[j * (int64_t)k + lane] : T(0);
    if (solver_mode == 1) {
        if (l1 > T(0) && fok) b -= l1;
        x = wave_chol_clip<T, KP>(Gl, b, k, nonneg, lane);
    } else {
        const T gd = Gl[ll * KP + ll];
        // static coordinate sweeps (cd_static_sweeps, kernels.hip.h): the lane's Gram column read from the wave's LDS tile at
        // compile-time offsets
        cd_static_sweeps<T, KP>(b, x, gd, fok, l1, nonneg, maxit, [&](auto IC) { return Gl[decltype(IC)::value * KP + ll]; });
    }
    if (fok) X[j * (int64_t)k + lane] = x;
}

// ---------------------------------------------------------------------------
// The same half-update with the Gram correction on the MATRIX cores (no user mask).  Held-out rows are collected in a small LDS
// queue (ballot + prefix popcount); every 32 of them are gathered with 16-byte loads, parked in LDS and applied as rank-2 (fp32)
// or rank-4 (fp64) updates  G_local -= f f^T  on an accumulator tile initialised with G (A operand = -f, B operand = f) --
// against k shuffles and k LDS read-modify-writes per held-out row in cv_solve_kernel.  With zeros held out a column of a
// 20 000-row matrix has ~2 000 such rows.
// The accumulators, their way to LDS and the CD solve are a Gram tile policy of mfma_gram_tile.hip.h; behind the tile's LDS
// (the staging area, aliased by G_local afterwards) stands the row queue.
// ---------------------------------------------------------------------------
constexpr int CV_QCAP = 96;   // row queue (ints): at most 31 rows waiting + 64 appended
// LDS elements of one wave: the host sizes the launch from it
template <class Tile> constexpr int cv_wave_elems = Tile::tile_elems + CV_QCAP * (int)sizeof(int) / (int)sizeof(typename Tile::Scalar);

template <class Tile>
__device__ __forceinline__ void cv_solve_mfma_body(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const typename Tile::Scalar* __restrict__ vals, int64_t ncols,
    int nrows, const typename Tile::Scalar* __restrict__ F, const typename Tile::Scalar* __restrict__ Gfull,
    typename Tile::Scalar* __restrict__ X, int k, unsigned long long seed, unsigned long long threshold, int mask_zeros,
    int transposed, typename Tile::Scalar l1, int nonneg, int maxit, int solver_mode) {
    typedef typename Tile::Scalar T;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* Gl = reinterpret_cast<T*>(smem_raw) + (size_t)wave * cv_wave_elems<Tile>;   // staged rows first, G_local [c][r] afterwards
    int* hq = reinterpret_cast<int*>(Gl + Tile::tile_elems);
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const bool fok = lane < k;
    const unsigned col = (unsigned)j;
    Tile tile(Gl, lane);
    tile.init(Gfull, k);
    int qn = 0;                                       // rows waiting in hq (wave-uniform)
    // append the rows flagged in `held` (one per lane, row index `row`) to the queue; flush while >= 32 are waiting
    auto push = [&](bool held, int row) {
        const unsigned long long m = __ballot(held);
        if (m == 0ull) return;
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (held) hq[qn + rank] = row;
        qn += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        while (qn >= 32) {
            tile.flush(32, hq, F, k);
            const int rest = qn - 32;
            const int moved = lane < rest ? hq[32 + lane] : 0;      // rest <= 63
            __builtin_amdgcn_wave_barrier();
            if (lane < rest) hq[lane] = moved;
            __builtin_amdgcn_wave_barrier();
            qn = rest;
        }
    };
    T b = T(0);
    for (int t0 = colptr[j]; t0 < colptr[j + 1]; t0 += 64) {       // 64 nonzeros per step: lane-parallel hashing
        const int t = t0 + lane;
        const bool valid = t < colptr[j + 1];
        const int row = valid ? rowidx[t] : 0;
        const T a = valid ? vals[t] : T(0);
        const bool held = valid && cv_held(seed, transposed, col, (unsigned)row, threshold);
        // train right-hand side: lane = feature again, one nonzero at a time
        unsigned long long tm = __ballot(valid && !held);
        while (tm) {
            const int bit = __builtin_ctzll(tm);
            tm &= tm - 1;
            const int rw = __builtin_amdgcn_readlane(row, bit);
            const T av = lane_value(a, bit);
            if (fok) b = tfma(av, F[(int64_t)rw * k + lane], b);
        }
        if (mask_zeros) push(held, row);
    }
    if (!mask_zeros) {
        for (int r0 = 0; r0 < nrows; r0 += 64) {
            const int rw = r0 + lane;
            const bool held = rw < nrows && cv_held(seed, transposed, col, (unsigned)rw, threshold);
            push(held, rw);
        }
    }
    if (qn > 0) tile.flush(qn, hq, F, k);
    tile.park(Gl, T(0), k);
    __builtin_amdgcn_wave_barrier();
    T x = fok ? X[j * (int64_t)k + lane] : T(0);
    if (solver_mode == 1) {
        if (l1 > T(0) && fok) b -= l1;
        x = wave_chol_clip<T, Tile::KP>(Gl, b, k, nonneg, lane);
    } else {
        tile.template solve_cd<false>(Gl, b, x, fok, l1, nonneg, maxit);
    }
    if (fok) X[j * (int64_t)k + lane] = x;
}

// the entry points, one per tile, each with its own occupancy hint (the 2 x 2 form: 64 KiB of LDS per block, two blocks per CU)
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void cv_solve_mfma32_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols, int nrows,
    const float* __restrict__ F, const float* __restrict__ Gfull, float* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, float l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<GramTile32>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
                               maxit, solver_mode);
}
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void cv_solve_mfma32x2_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols, int nrows,
    const float* __restrict__ F, const float* __restrict__ Gfull, float* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, float l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<GramTile32x2>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
                                 maxit, solver_mode);
}
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void cv_solve_mfma64_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ vals, int64_t ncols, int nrows,
    const double* __restrict__ F, const double* __restrict__ Gfull, double* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, double l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<GramTile64>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
                               maxit, solver_mode);
}

// Squared error and count over the held-out entries (fit_cv.hpp:1444-1494), one wavefront per column of A.
// out partials: [block] = {sum of squared errors (fp64), count}
template <class T>
__global__ __launch_bounds__(256) void cv_test_error_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const T* __restrict__ vals, int64_t ncols, int nrows,
    const T* __restrict__ W_T, const T* __restrict__ d, const T* __restrict__ H, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, double* __restrict__ partial_sq, unsigned long long* __restrict__ partial_n) {
    __shared__ double shs[4];
    __shared__ unsigned long long shn[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    double acc = 0.0;
    unsigned long long cnt = 0;
    if (j < ncols) {
        const bool fok = lane < k;
        // lane f holds d_f * H(f, j) for features f and f + 64 (k <= 128); a held-out entry costs one gather of W_T(row, :) and a
        // wave reduction
        const bool fok2 = lane + 64 < k;
        const T hd = fok ? H[j * (int64_t)k + lane] * d[lane] : T(0);
        const T hd2 = fok2 ? H[j * (int64_t)k + lane + 64] * d[lane + 64] : T(0);
        const unsigned col = (unsigned)j;
        if (mask_zeros) {
            for (int t = colptr[j]; t < colptr[j + 1]; ++t) {
                const int row = rowidx[t];
                if (!cv_held(seed, 0, col, (unsigned)row, threshold)) continue;
                T p = fok ? W_T[(int64_t)row * k + lane] * hd : T(0);
                if (fok2) p = tfma(W_T[(int64_t)row * k + lane + 64], hd2, p);
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) p += shfl_xor_t(p, off);
                const T diff = vals[t] - p;
                acc += static_cast<double>(diff * diff);
                ++cnt;
            }
        } else {
            int t = colptr[j];
            const int te = colptr[j + 1];
            for (int r0 = 0; r0 < nrows; r0 += 64) {
                const int r = r0 + lane;
                const bool held = r < nrows && cv_held(seed, 0, col, (unsigned)r, threshold);
                unsigned long long m = __ballot(held);
                while (m) {
                    const int bit = __builtin_ctzll(m);
                    m &= m - 1;
                    const int row = r0 + bit;
                    while (t < te && rowidx[t] < row) ++t;
                    const T actual = (t < te && rowidx[t] == row) ? vals[t] : T(0);
                    T p = fok ? W_T[(int64_t)row * k + lane] * hd : T(0);
                    if (fok2) p = tfma(W_T[(int64_t)row * k + lane + 64], hd2, p);
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) p += shfl_xor_t(p, off);
                    const T diff = actual - p;
                    acc += static_cast<double>(diff * diff);
                    ++cnt;
                }
            }
        }
    }
    if (lane == 0) { shs[wave] = acc; shn[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_sq[blockIdx.x] = shs[0] + shs[1] + shs[2] + shs[3];
        partial_n[blockIdx.x] = shn[0] + shn[1] + shn[2] + shn[3];
    }
}

}  // namespace rk
