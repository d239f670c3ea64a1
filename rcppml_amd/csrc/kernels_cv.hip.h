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
#include "kernels.hip.h"

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
//
// A tile policy owns the accumulators of one wave and says how they meet LDS:
//   Scalar, KP (padded rank of G_local), FS (stride of a staged row), tile_elems, wave_elems (LDS elements of one wave: the
//   staging area, aliased by G_local afterwards, then the row queue -- the host sizes the launch from it);
//   init(Gfull, k), flush(cnt, hq, F, k) (apply the first cnt <= 32 queued rows), park(Gl) (G_local to LDS, [c][r]) and
//   solve_cd(Gl, b, x, ...).
// ---------------------------------------------------------------------------
constexpr int CV_QCAP = 96;   // row queue (ints): at most 31 rows waiting + 64 appended

// fp32, k <= 32 (k % 4 == 0): one 32 x 32 tile, v_mfma_f32_32x32x2_f32; staging: lane = row t, feature half hh
struct CvTile32 {
    typedef float Scalar;
    static constexpr int KP = 32, FS = 36;
    static constexpr int tile_elems = 32 * FS, wave_elems = tile_elems + CV_QCAP;
    float* Fst;
    int lane, r, hh;
    f32x16 acc;
    __device__ __forceinline__ CvTile32(float* st, int lane_) : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5) {}
    __device__ __forceinline__ void init(const float* __restrict__ Gfull, int k) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh, gj = r;
            acc[v] = (gi < k && gj < k) ? Gfull[(int64_t)gj * k + gi] : (gi == gj ? 1.f : 0.f);
        }
    }
    __device__ __forceinline__ void flush(int cnt, const int* hq, const float* __restrict__ F, int k) {
        const bool ok = r < cnt;
        const int row = ok ? hq[r] : 0;
        const float* fsrc = F + (int64_t)row * k + 16 * hh;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c0 = 16 * hh + 4 * q;
            const float4 v = (ok && c0 < k) ? *reinterpret_cast<const float4*>(fsrc + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Fst + r * FS + c0) = v;
        }
        __builtin_amdgcn_wave_barrier();
        const int nst = (cnt + 1) >> 1;
#pragma unroll 4
        for (int s2 = 0; s2 < nst; ++s2) {
            const float fv = Fst[(2 * s2 + hh) * FS + r];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(-fv, fv, acc, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void park(float* Gl) const {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh;
            Gl[gi * KP + r] = acc[v];
        }
    }
    // the lane's column of the corrected Gram in registers: the sweep picks row i with a wave-uniform register-indexed
    // move instead of an LDS read on the dependent chain of every step (as irls_nb_mfma32_kernel does)
    __device__ __forceinline__ void solve_cd(const float* Gl, float& b, float& x, bool fok, float l1, int nonneg, int maxit) const {
        const int ll = lane < KP ? lane : 0;
        const float gd = Gl[ll * KP + ll];
        typedef float f32x32 __attribute__((ext_vector_type(32)));
        f32x32 gcol;
#pragma unroll
        for (int c = 0; c < KP; ++c) gcol[c] = Gl[c * KP + ll];
        float gg[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) gg[c] = gcol[c];
        cd_static_sweeps_scaled_f32<KP>(b, x, gd, fok, l1, nonneg, maxit, gg);
    }
};

// fp32, 32 < k <= 64 (k % 4 == 0): a 2 x 2 grid of 32 x 32 tiles (three MFMAs per pair of held-out rows; the lower-left tile is
// the transpose of the upper-right one and is never computed), lane = feature over the whole wave in the solve; 16 KiB of LDS
// per wave for G_local, whose head doubles as the 32 x FS staging area (two blocks per CU)
struct CvTile32x2 {
    typedef float Scalar;
    static constexpr int KP = 64, FS = 68;
    static constexpr int tile_elems = KP * KP, wave_elems = tile_elems + CV_QCAP;
    float* Fst;
    int lane, r, hh;
    f32x16 a00, a01, a11;
    __device__ __forceinline__ CvTile32x2(float* st, int lane_) : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5) {}
    __device__ __forceinline__ void init(const float* __restrict__ Gfull, int k) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh, gj = r;
            auto base = [&](int i2, int j2) { return (i2 < k && j2 < k) ? Gfull[(int64_t)j2 * k + i2] : (i2 == j2 ? 1.f : 0.f); };
            a00[v] = base(gi, gj); a01[v] = base(gi, gj + 32); a11[v] = base(gi + 32, gj + 32);
        }
    }
    __device__ __forceinline__ void flush(int cnt, const int* hq, const float* __restrict__ F, int k) {
        const bool ok = r < cnt;
        const int row = ok ? hq[r] : 0;
        const float* fsrc = F + (int64_t)row * k + 32 * hh;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c0 = 32 * hh + 4 * q;
            const float4 v = (ok && c0 < k) ? *reinterpret_cast<const float4*>(fsrc + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(Fst + r * FS + c0) = v;
        }
        __builtin_amdgcn_wave_barrier();
        const int nst = (cnt + 1) >> 1;
#pragma unroll 2
        for (int s2 = 0; s2 < nst; ++s2) {
            const float f0 = Fst[(2 * s2 + hh) * FS + r], f1 = Fst[(2 * s2 + hh) * FS + 32 + r];
            a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(-f0, f0, a00, 0, 0, 0);
            a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(-f0, f1, a01, 0, 0, 0);
            a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(-f1, f1, a11, 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void park(float* Gl) const {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh;
            Gl[gi * KP + r] = a00[v];
            Gl[gi * KP + 32 + r] = a01[v];                    // G(row gi, col 32 + r) and its mirror
            Gl[(32 + r) * KP + gi] = a01[v];
            Gl[(gi + 32) * KP + 32 + r] = a11[v];
        }
    }
    // as CvTile32::solve_cd, the column in two halves: hipcc indexes 32-element vectors with s_set_gpr_idx, 64-element ones
    // through scratch
    __device__ __forceinline__ void solve_cd(const float* Gl, float& b, float& x, bool fok, float l1, int nonneg, int maxit) const {
        const int ll = lane;
        const float gd = Gl[ll * KP + ll];
        typedef float f32x32 __attribute__((ext_vector_type(32)));
        f32x32 gcol0, gcol1;
#pragma unroll
        for (int c = 0; c < 32; ++c) { gcol0[c] = Gl[c * KP + ll]; gcol1[c] = Gl[(32 + c) * KP + ll]; }
        float gg[KP];
#pragma unroll
        for (int c = 0; c < 32; ++c) { gg[c] = gcol0[c]; gg[32 + c] = gcol1[c]; }
        cd_static_sweeps_scaled_f32<KP>(b, x, gd, fok, l1, nonneg, maxit, gg);
    }
};

// fp64, k <= 32 (k % 2 == 0): 2 x 2 tiles of 16 x 16, v_mfma_f64_16x16x4_f64 (four held-out rows per instruction step, C/D map
// col = lane&15, row = (lane>>4) + 4v); MFMA phase: feature slot r16, K-slot kk
struct CvTile64 {
    typedef double Scalar;
    static constexpr int KP = 32, FS = 34;
    static constexpr int tile_elems = 32 * FS, wave_elems = tile_elems + CV_QCAP / 2;
    double* Fst;
    int lane, r, hh, r16, kk;
    f64x4 acc[2][2];
    __device__ __forceinline__ CvTile64(double* st, int lane_)
        : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5), r16(lane_ & 15), kk(lane_ >> 4) {}
    __device__ __forceinline__ void init(const double* __restrict__ Gfull, int k) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int gi = 16 * ti + kk + 4 * v, gj = 16 * tj + r16;
                    acc[ti][tj][v] = (gi < k && gj < k) ? Gfull[(int64_t)gj * k + gi] : (gi == gj ? 1.0 : 0.0);
                }
    }
    __device__ __forceinline__ void flush(int cnt, const int* hq, const double* __restrict__ F, int k) {
        const bool ok = r < cnt;
        const int row = ok ? hq[r] : 0;
        const double* fsrc = F + (int64_t)row * k + 16 * hh;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c0 = 16 * hh + 2 * q;
            const double2 v = (ok && c0 < k) ? *reinterpret_cast<const double2*>(fsrc + 2 * q) : make_double2(0.0, 0.0);
            *reinterpret_cast<double2*>(Fst + r * FS + c0) = v;
        }
        __builtin_amdgcn_wave_barrier();
        const int nst = (cnt + 3) >> 2;
#pragma unroll 2
        for (int s4 = 0; s4 < nst; ++s4) {
            const int t = 4 * s4 + kk;
            const double f0 = Fst[t * FS + r16], f1 = Fst[t * FS + 16 + r16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-f0, f0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-f0, f1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(-f1, f0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(-f1, f1, acc[1][1], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ void park(double* Gl) const {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v) Gl[(16 * ti + kk + 4 * v) * KP + 16 * tj + r16] = acc[ti][tj][v];
    }
    // static coordinate sweeps (cd_static_sweeps, kernels.hip.h), the lane's Gram column read from the wave's LDS tile
    __device__ __forceinline__ void solve_cd(const double* Gl, double& b, double& x, bool fok, double l1, int nonneg, int maxit) const {
        const int ll = lane < KP ? lane : 0;
        const double gd = Gl[ll * KP + ll];
        cd_static_sweeps<double, KP>(b, x, gd, fok, l1, nonneg, maxit, [&](auto IC) { return Gl[decltype(IC)::value * KP + ll]; });
    }
};

template <class Tile>
__device__ __forceinline__ void cv_solve_mfma_body(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const typename Tile::Scalar* __restrict__ vals, int64_t ncols,
    int nrows, const typename Tile::Scalar* __restrict__ F, const typename Tile::Scalar* __restrict__ Gfull,
    typename Tile::Scalar* __restrict__ X, int k, unsigned long long seed, unsigned long long threshold, int mask_zeros,
    int transposed, typename Tile::Scalar l1, int nonneg, int maxit, int solver_mode) {
    typedef typename Tile::Scalar T;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* Gl = reinterpret_cast<T*>(smem_raw) + (size_t)wave * Tile::wave_elems;   // staged rows first, G_local [c][r] afterwards
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
    tile.park(Gl);
    __builtin_amdgcn_wave_barrier();
    T x = fok ? X[j * (int64_t)k + lane] : T(0);
    if (solver_mode == 1) {
        if (l1 > T(0) && fok) b -= l1;
        x = wave_chol_clip<T, Tile::KP>(Gl, b, k, nonneg, lane);
    } else {
        tile.solve_cd(Gl, b, x, fok, l1, nonneg, maxit);
    }
    if (fok) X[j * (int64_t)k + lane] = x;
}

// the entry points, one per tile, each with its own occupancy hint (the 2 x 2 form: 64 KiB of LDS per block, two blocks per CU)
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void cv_solve_mfma32_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols, int nrows,
    const float* __restrict__ F, const float* __restrict__ Gfull, float* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, float l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<CvTile32>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
                               maxit, solver_mode);
}
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void cv_solve_mfma32x2_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols, int nrows,
    const float* __restrict__ F, const float* __restrict__ Gfull, float* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, float l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<CvTile32x2>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
                                 maxit, solver_mode);
}
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void cv_solve_mfma64_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ vals, int64_t ncols, int nrows,
    const double* __restrict__ F, const double* __restrict__ Gfull, double* __restrict__ X, int k, unsigned long long seed,
    unsigned long long threshold, int mask_zeros, int transposed, double l1, int nonneg, int maxit, int solver_mode) {
    cv_solve_mfma_body<CvTile64>(colptr, rowidx, vals, ncols, nrows, F, Gfull, X, k, seed, threshold, mask_zeros, transposed, l1, nonneg,
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
