// ============================================================================
// kernels_irls.hip.h -- IRLS weights and half-update (solve) kernels of the ALS-NNLS NMF update for gfx950
// (BASELINE config 5).  The dispersion estimators and likelihoods: kernels_dispersion.hip.h.
//
//   irls_weight_*_dev     math/loss.hpp:176-303, nnls_batch_irls.hpp:57-120
//   irls_nb_solve_kernel  primitives/cpu/nnls_batch_irls.hpp:202-329,465-520 (any k <= 64, row-in-registers weighted Gram)
//   irls_nb_mfma*_kernel  the same half-update with the weighted Gram on the matrix cores
//
// One wavefront per column, lane r = feature r (k <= 64).  Per IRLS pass the wave walks the column's nonzeros once:
// the reconstruction f_i . x is a wave reduction, the NB weight is evaluated in fp64 as the reference does, and the
// weighted Gram  G_w = G + sum (w-1) f f^T  is accumulated ROW-WISE IN REGISTERS (lane r keeps row r, k VGPRs;
// f_c is broadcast with v_readlane) -- no LDS traffic in the O(nnz_j k^2) part.  G_w is then parked in LDS
// ([c][r], this wave's tile) for the coordinate-descent solve, which is the exact sequential sweep of
// cd_nnls_col_fixed with ballot skipping of no-op coordinates (all cd_maxit sweeps: the reference passes cd_tol = 0).
// ============================================================================
#pragma once
#include "mfma_gram_tile.hip.h"

namespace rk {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}


// value of lane I of the caller's 16-lane DPP row, in every lane of that row (row_newbcast, gfx90a+; folds into a VOP2 consumer)
template <int I> __device__ __forceinline__ float row_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + I, 0xf, 0xf, true));
}
// d0 += g0 * s, d1 += g1 * s with s = lane I of the row's `src`: two v_fmac_f32 with the DPP broadcast folded into their first
// operand.  (hipcc emits v_mov_b32_dpp + two fmacs for the builtin, and defers / spills the broadcasts of a half sweep.)  The
// s_nop covers the two wait states a DPP read needs after the VALU write of `src`.
template <int I> __device__ __forceinline__ void row_fmac2(float& d0, float& d1, float src, float g0, float g1) {
    asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %2, %3 row_newbcast:%5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f32_dpp %1, %2, %4 row_newbcast:%5 row_mask:0xf bank_mask:0xf"
                 : "+v"(d0), "+v"(d1) : "v"(src), "v"(g0), "v"(g1), "n"(I));
}

template <int I> __device__ __forceinline__ int row_bcast_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x150 + I, 0xf, 0xf, true); }
// sum over the eight lanes 8g .. 8g+7 of v, left in all eight (quad_perm xor 1, xor 2, then row_half_mirror: the other quad's sum)
__device__ __forceinline__ float sum8(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true));     // quad_perm:[1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true));     // quad_perm:[2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, true));    // row_half_mirror
    return v;
}

// One coordinate of a half sweep of the four-columns-per-wave CD solve, as ONE instruction group (see irls_nb_mfma32q_kernel):
//   step = med3(dc, -x, inf);  do += go_prev * bcast(step_prev);  own = turn ? step : own;  dc += gc * bcast(step)
// dc is the residual this half's steps are read from, `do` the other one (its update for the PREVIOUS coordinate, deferred by
// one so that two independent operations separate the med3 from the DPP read of its result: no s_nop).
template <int I> __device__ __forceinline__ float sweep_step(float& dc, float& dother, float& own, float step_prev, float nxe, float inf,
                                                             unsigned long long turn, float gc, float go_prev) {
    float step;
    asm volatile("v_med3_f32 %0, %1, %4, %5\n\t"
                 "v_fmac_f32_dpp %2, %6, %8 row_newbcast:%10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_cndmask_b32_e64 %3, %3, %0, %9\n\t"
                 "v_fmac_f32_dpp %1, %0, %7 row_newbcast:%11 row_mask:0xf bank_mask:0xf"
                 : "=&v"(step), "+v"(dc), "+v"(dother), "+v"(own)
                 : "v"(nxe), "v"(inf), "v"(step_prev), "v"(gc), "v"(go_prev), "s"(turn), "n"(I - 1), "n"(I));
    return step;
}
// the first coordinate of a half: nothing deferred yet, one wait state filled by an s_nop
template <int I> __device__ __forceinline__ float sweep_first(float& dc, float& own, float nxe, float inf, unsigned long long turn, float gc) {
    float step;
    asm volatile("v_med3_f32 %0, %1, %3, %4\n\t"
                 "v_cndmask_b32_e64 %2, %2, %0, %6\n\t"
                 "s_nop 0\n\t"
                 "v_fmac_f32_dpp %1, %0, %5 row_newbcast:%7 row_mask:0xf bank_mask:0xf"
                 : "=&v"(step), "+v"(dc), "+v"(own)
                 : "v"(nxe), "v"(inf), "v"(gc), "s"(turn), "n"(I));
    return step;
}
template <int I> __device__ __forceinline__ void row_fmac1(float& d, float src, float g) {
    asm volatile("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(src), "v"(g), "n"(I));
}

// math/loss.hpp:248-256  irls_weight_nb: computed in double, eps = tiny_num<Scalar>() = Scalar(1e-15)
template <class T> __device__ __forceinline__ T irls_weight_nb_dev(T predicted, T nb_size) {
    double mu = static_cast<double>(predicted);
    const double eps = static_cast<double>(static_cast<T>(1e-15));
    mu = mu > eps ? mu : eps;
    double r = static_cast<double>(nb_size);
    r = r > 1e-10 ? r : 1e-10;
    double w = r / (mu * (r + mu));
    w = w < 1e6 ? w : 1e6;
    return static_cast<T>(w);
}

// distribution weight of the two implemented IRLS losses (nnls_batch_irls.hpp:57-83): 5 = NB; 4 = GP, whose W/H
// updates use the KL weight 1 / max(mu, 1e-4) in Scalar arithmetic (fit_cpu.hpp:568-574, math/loss.hpp:176-179)
// 6 / 7 / 8 = Gamma / inverse Gaussian / Tweedie: power-variance weight min(1/mu^p, 1e6) in fp64 (math/loss.hpp:270-278)
template <class T> __device__ __forceinline__ T irls_weight_dev(int loss_type, T predicted, T theta, T power) {
    if (loss_type == 4) return T(1) / (predicted > T(1e-4) ? predicted : T(1e-4));
    if (loss_type >= 6) {
        double mu = static_cast<double>(predicted);
        const double eps = static_cast<double>(static_cast<T>(1e-15));
        mu = mu > eps ? mu : eps;
        const double p = loss_type == 6 ? 2.0 : (loss_type == 7 ? 3.0 : static_cast<double>(power));
        double w = 1.0 / pow(mu, p);
        w = w < 1e6 ? w : 1e6;
        return static_cast<T>(w);
    }
    return irls_weight_nb_dev<T>(predicted, theta);
}

// math/loss.hpp:294-303  the distribution weight times the Huber modifier of the Pearson residual when robust_delta > 0
template <class T> __device__ __forceinline__ T huber_weight_dev(T w_dist, T residual, T robust) {
    if (robust > T(0)) {
        const T wd = w_dist > T(1e-15) ? w_dist : T(1e-15);
        const T abs_r = tabs(residual * sqrt(wd));
        return abs_r <= robust ? w_dist : w_dist * (robust / (abs_r + T(1e-15)));
    }
    return w_dist;
}

// nnls_batch_irls.hpp:95-120  compute_irls_weight: distribution weight (1 for loss_type 0 = MSE) x Huber modifier
template <class T> __device__ __forceinline__ T irls_weight_full_dev(int loss_type, T residual, T predicted, T theta, T power,
                                                                     T robust) {
    return huber_weight_dev<T>(loss_type == 0 ? T(1) : irls_weight_dev<T>(loss_type, predicted, theta, power), residual, robust);
}

template <class T, int KP>   // KP in {32, 64}: features padded to KP (k <= KP), lane r = feature r
__global__ __launch_bounds__(256) void irls_nb_solve_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const T* __restrict__ vals, int64_t ncols,
    const T* __restrict__ F, const T* __restrict__ Gbase, T* __restrict__ X, int k, T l1, T l2, int nonneg,
    int cd_maxit, int irls_max_iter, T irls_tol, const T* __restrict__ theta_row, const T* __restrict__ theta_col,
    int loss_type, T power, T robust,
    unsigned long long* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* Gl = reinterpret_cast<T*>(smem_raw) + (size_t)wave * KP * KP;    // [c][r]
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const bool fok = lane < k;
    const bool lin = lane < KP;                  // KP = 32: the upper half of the wave only takes part in shuffles
    const int ll = lin ? lane : 0;
    // base Gram row r in registers (padded with identity)
    T gb[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) gb[c] = (fok && c < k) ? Gbase[(int64_t)c * k + lane] : (c == lane ? T(1) : T(0));
    const int as = colptr[j], ae = colptr[j + 1];
    const T th_col = theta_col ? theta_col[j] : T(0);
    T x = T(0);                                   // nnls_batch_irls.hpp:482-483  H.setZero(): no warm start
    int passes = 0, nsw = 0;      // IRLS passes; CD sweeps executed over all passes (work counters)
    for (int irls = 0; irls < irls_max_iter; ++irls) {
        ++passes;
        T gw[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) gw[c] = gb[c];
        T bw = T(0);
        for (int t = as; t < ae; ++t) {
            const int row = rowidx[t];
            const T a = vals[t];
            const T fr = fok ? F[(int64_t)row * k + lane] : T(0);
            const T recon = wave_sum(fr * x);                                   // W_T.col(row).dot(x)
            const T th = theta_col ? th_col : (theta_row ? theta_row[row] : T(0));
            const T w = irls_weight_full_dev<T>(loss_type, a - recon, recon, th, power, robust);
            const T dw = w - T(1);
            const T wv = w * a;
            const T frd = fr * dw;                                              // W_nnz_scaled.col = W_block.col * dw
#pragma unroll
            for (int c = 0; c < KP; ++c) {
                const T fc = __shfl(fr, c, 64);
                gw[c] = tfma(frd, fc, gw[c]);                                   // G_w(r,c) += (f_r dw) f_c
            }
            bw = tfma(fr, wv, bw);                                              // b_w += f * (w a)
        }
        if (l2 > T(0)) {
#pragma unroll
            for (int c = 0; c < KP; ++c)
                if (c == lane && fok) gw[c] += l2;
        }
        // park G_w in LDS; residual b_c = b_w - G_w x_old
        const T x_old = x;
        T b = bw;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            if (lin) Gl[c * KP + lane] = gw[c];
            const T xc = __shfl(x_old, c, 64);
            b = tfma(-gw[c], xc, b);
        }
        const T gd = Gl[ll * KP + ll];
        // cd_nnls_col_fixed(G_w, b_c, x, L1 inside, L2 = 0, nonneg, cd_maxit, ub = 0, tol = 0): all sweeps
        // static coordinate sweeps (cd_static_sweeps, kernels.hip.h): the lane's Gram column read from the wave's LDS tile at
        // compile-time offsets
        nsw += cd_static_sweeps<T, KP>(b, x, gd, fok, l1, nonneg, cd_maxit, [&](auto IC) { return Gl[decltype(IC)::value * KP + ll]; });
        // IRLS convergence: max_i |x_i - x_old_i| / (|x_old_i| + 1e-12) < irls_tol
        T rel = fok ? tabs(x - x_old) / (tabs(x_old) + T(1e-12)) : T(0);
        rel = wave_max(rel);
        if (rel < irls_tol) break;
    }
    if (fok) X[j * (int64_t)k + lane] = x;
    // work counters (RCPPML_OPT_CD_COUNT_NOOP only): IRLS passes and nonzero-passes = weighted-Gram rank-1 updates
    if (stats && lane == 0) { atomicAdd(stats, (unsigned long long)passes); atomicAdd(stats + 1, (unsigned long long)passes * (unsigned long long)(ae - as)); atomicAdd(stats + 4, (unsigned long long)nsw); }
}

// ---------------------------------------------------------------------------
// fp32, k <= 32 (k % 4 == 0): the same IRLS half-update with the weighted Gram on the MATRIX cores.
//   G_w = G + F_nz diag(w - 1) F_nz^T  is a rank-nnz_j update of a 32 x 32 tile: two nonzeros fill the two K-slots of one
//   v_mfma_f32_32x32x2_f32 (A operand = (w_t - 1) f_t, B operand = f_t), against 32 shuffles + 32 fmas per nonzero in the
//   row-in-registers form above.  The column is processed in chunks of 32 nonzeros:
//   phase A (lane = nonzero t, half h of its features): coalesced (row, value) load, 16-byte gathers of F(row, :), the
//     reconstruction f_t . x as 16 in-lane fmas + one half swap, the NB weight in fp64 -- all 32 nonzeros IN PARALLEL
//     (the wave-per-nonzero form evaluates one weight per 64 lanes) -- and f_t, (w_t - 1), w_t a_t parked in LDS;
//   phase B (lane = feature r, K-slot kk): one conflict-free ds_read_b32 of f_t[r] per lane feeds both MFMA operands and
//     the weighted right-hand side b_w[r] += w_t a_t f_t[r].
//   The CD solve is unchanged (exact sequential sweep with ballot skipping); G_w is written from the accumulator tile
//   straight into its LDS slab, which aliases the staging buffer.
// ---------------------------------------------------------------------------
// LDS elements of one wave of the one-column kernels below: the tile's staging area (G_w afterwards) | (w - 1, w a) pairs | x.
// The kernels lay their LDS out with it and the host sizes the launches from it.
template <class Tile> constexpr int irls_wave_elems = Tile::tile_elems + 2 * Tile::CH + Tile::KP;
static_assert(irls_wave_elems<GramTile32> == 32 * 36 + 2 * 32 + 32, "LDS layout of irls_nb_mfma32_kernel");
static_assert(irls_wave_elems<GramTile32x2> == 64 * 64 + 2 * 32 + 64, "LDS layout of irls_nb_mfma32x2_kernel");
static_assert(irls_wave_elems<GramTile64> == 32 * 34 + 2 * 32 + 32, "LDS layout of irls_nb_mfma64_kernel");
// LT >= 0: the loss is known at compile time and there is no robust modifier (LT = 5: negative binomial, what C5 runs) -- the
// weight function then holds neither the fp64 pow() of the power-variance losses nor the Huber branch, whose registers the
// generic instantiation (LT = -1) pays for in every lane whatever loss it runs (64-VGPR budget at eight waves per SIMD).
template <int LT>
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void irls_nb_mfma32_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols,
    const float* __restrict__ F, const float* __restrict__ Gbase, float* __restrict__ X, int k, float l1, float l2,
    int nonneg, int cd_maxit, int irls_max_iter, float irls_tol, const float* __restrict__ theta_row,
    const float* __restrict__ theta_col, int loss_type, float power, float robust,
    unsigned long long* __restrict__ stats) {
    constexpr int KP = GramTile32::KP, CH = GramTile32::CH, FS = GramTile32::FS;   // FS: padded row stride of the staged F rows
    constexpr int WAVE_FLOATS = irls_wave_elems<GramTile32>;  // staged rows | (w-1, w a) pairs | x
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* Fst = reinterpret_cast<float*>(smem_raw) + (size_t)wave * WAVE_FLOATS;
    float2* sc = reinterpret_cast<float2*>(Fst + CH * FS);
    float* xs = Fst + CH * FS + 2 * CH;
    float* Gl = Fst;                                    // [c][r], KP*KP <= CH*FS: reused once the Gram is complete
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const int r = lane & 31, hh = lane >> 5;            // phase A: nonzero r, feature half hh; phase B: feature r, K-slot hh
    const int g8 = lane >> 3, p8 = lane & 7;            // gather: group of eight lanes = one row of F, lane = 16-byte piece
    const bool pok = 4 * p8 < k;
    const char* Fp = reinterpret_cast<const char*>(F) + 16 * p8;    // the lane's piece of row 0
    const bool fok = lane < k;
    const bool lin = lane < KP;
    const int ll = lin ? lane : 0;
    const int as = colptr[j], ae = colptr[j + 1];
    const float th_col = theta_col ? theta_col[j] : 0.f;
    float x = 0.f;                                      // nnls_batch_irls.hpp:482-483  H.setZero(): no warm start
    int passes = 0, nsw = 0;      // IRLS passes; CD sweeps executed over all passes (work counters)
    for (int irls = 0; irls < irls_max_iter; ++irls) {
        ++passes;
        GramTile32 tile(Fst, lane);                     // accumulator tile <- base Gram, 16-byte loads
        tile.init_vec4(Gbase, k);
        if (lin) xs[lane] = x;
        float bw = 0.f;
        __builtin_amdgcn_wave_barrier();
        const float4 xq = *reinterpret_cast<const float4*>(xs + 4 * p8);    // the lane's piece of x
        for (int t0 = as; t0 < ae; t0 += CH) {
            // ---- phase A.  Gather: the eight lanes 8g .. 8g+7 read the eight 16-byte pieces of ONE row of F (one 128-byte line per
            // group and instruction, eight lines per instruction against 32 for a lane-per-row layout); instruction i of group g takes
            // chunk row 4g + i.  The reconstruction f . x is four in-lane fmas against the lane's piece of x and a sum over the group.
            // (a lane past the column's end takes the position of the column's LAST nonzero: a valid row of F, no branch around
            //  the loads; its weight pair is (0, 0), so it adds exact zeros to G_w and b_w all the same)
            const int tt = t0 + r;
            const bool ok = tt < ae;
            const int tc = ok ? tt : ae - 1;
            const int row = rowidx[tc];
            const float a = ok ? vals[tc] : 0.f;
            float mine = 0.f;
            float4 fv4[4];
            if (k == KP) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned rowg = (unsigned)__shfl(row, 4 * g8 + i, 64);  // row of the chunk: 4g + i
                    fv4[i] = *reinterpret_cast<const float4*>(Fp + ((unsigned long long)rowg << 7));
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned rowg = (unsigned)__shfl(row, 4 * g8 + i, 64);
                    fv4[i] = pok ? *reinterpret_cast<const float4*>(Fp + (unsigned long long)rowg * (unsigned)(4 * k)) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float part = fv4[i].x * xq.x;
                part = tfma(fv4[i].y, xq.y, part);
                part = tfma(fv4[i].z, xq.z, part);
                part = tfma(fv4[i].w, xq.w, part);
                part = sum8(part);                                               // W_T.col(row).dot(x), in the group's eight lanes
                mine = (p8 & 3) == i ? part : mine;
                *reinterpret_cast<float4*>(Fst + (4 * g8 + i) * FS + 4 * p8) = fv4[i];
            }
            const float recon = __shfl(mine, 8 * (r >> 2) + (r & 3), 64);        // row r of the chunk: group r / 4, instruction r % 4
            const float th = theta_col ? th_col : (theta_row ? theta_row[row] : 0.f);
            const float w = irls_weight_full_dev<float>(LT >= 0 ? LT : loss_type, a - recon, recon, th, power, LT >= 0 ? 0.f : robust);
            if (hh == 0) sc[r] = make_float2(ok ? w - 1.f : 0.f, ok ? w * a : 0.f);
            __builtin_amdgcn_wave_barrier();
            tile.update_staged(ae - t0 < CH ? ae - t0 : CH, sc, bw);         // ---- phase B
            __builtin_amdgcn_wave_barrier();
        }
        bw += __shfl_xor(bw, 32, 64);
        // park G_w in LDS ([c][r]; symmetric, so accumulator row i is written as slab row i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh;
            float val = tile.acc[v];
            if (l2 > 0.f && gi == r && gi < k) val += l2;
            Gl[gi * KP + r] = val;
        }
        __builtin_amdgcn_wave_barrier();
        // residual b_c = b_w - G_w x_old
        // (the lane keeps ITS column of G_w -- G_w(c, ll), c = 0..31 -- in registers: the sweep below picks row i of it with a
        //  wave-uniform index, i.e. a register-indexed move instead of an LDS read on the dependent chain of every step)
        const float x_old = x;
        float b = bw;
        typedef float f32x32 __attribute__((ext_vector_type(32)));
        f32x32 gcol;
#pragma unroll
        for (int c = 0; c < KP; ++c) {
            const float xc = __shfl(x_old, c, 64);
            const float gv = Gl[c * KP + ll];
            gcol[c] = gv;
            b = tfma(-gv, xc, b);
        }
        const float gd = Gl[ll * KP + ll];
        // cd_nnls_col_fixed(G_w, b_c, x, L1 inside, L2 = 0, nonneg, cd_maxit, ub = 0, tol = 0): all sweeps, static form (kernels.hip.h)
        {
            float gg[KP];
#pragma unroll
            for (int c = 0; c < KP; ++c) gg[c] = gcol[c];
            nsw += cd_static_sweeps_scaled_f32<KP>(b, x, gd, fok, l1, nonneg, cd_maxit, gg);
        }
        float rel = fok ? tabs(x - x_old) / (tabs(x_old) + 1e-12f) : 0.f;
        rel = wave_max(rel);
        __builtin_amdgcn_wave_barrier();
        if (rel < irls_tol) break;
    }
    if (fok) X[j * (int64_t)k + lane] = x;
    // work counters (RCPPML_OPT_CD_COUNT_NOOP only): IRLS passes and nonzero-passes = weighted-Gram rank-1 updates
    if (stats && lane == 0) { atomicAdd(stats, (unsigned long long)passes); atomicAdd(stats + 1, (unsigned long long)passes * (unsigned long long)(ae - as)); atomicAdd(stats + 4, (unsigned long long)nsw); }
}

// ---------------------------------------------------------------------------
// fp32, k <= 32 (k % 4 == 0), MANY columns (H side of C5: 200 000 columns of ~190 nonzeros): FOUR columns per wavefront.
// The CD solve of the kernel above spends 4 VALU operations per coordinate and sweep with half of the wave's lanes idle
// (k = 32) and one column in flight; it is VALU-issue bound there (the solves are half of the H side's time).  Here the solve
// puts one column on each 16-lane DPP row, a lane holding TWO coordinates (l and l + 16) and the two matching rows of its
// column's scaled Gram (64 registers): coordinate i's step is broadcast inside every row at once by DPP row_newbcast folded
// into the consuming v_fmac (no v_readlane / SGPR round trip), so one coordinate costs med3 + 2 fmac_dpp + 1 select for
// FOUR columns instead of four operations for one.  The weighted Grams of the four columns are built one after the other by
// the whole wave exactly as above (MFMA, chunks of 64 nonzeros = two phase-A halves so that every lane evaluates ONE NB
// weight -- in the kernel above both halves of the wave evaluate the same 32), parked in the wave's LDS slab and picked up by
// the column's row (columns l and l + 16 of the slab: 64 four-byte reads, conflict-free).
// Steps, their order and the arithmetic of a column are those of irls_nb_mfma32_kernel: results are bit-identical to it
// (tests/test_gpu_nb.py::test_quad_equals_single).  A column that converged keeps its iterate: its row holds a zero Gram and a
// zero residual from then on, so the sweeps the other columns still need do not move it.
// 128 VGPRs (four waves per SIMD = 16 columns per SIMD against 8), 9.75 KiB of LDS per wave.
// The tile's init and update are the shared ones (the update reads whatever rows are staged: 64 here); phase A, the park (the
// slab is [col][row] with stride FS, written and picked up with 16-byte accesses) and the DPP solve are this kernel's own.
// ---------------------------------------------------------------------------
constexpr int IRLS_QUAD_CH = 64;
// LDS of one wave: staged rows / G_w slab | (w-1, w a) pairs | x | b_w
constexpr int IRLS_QUAD_WAVE_ELEMS = IRLS_QUAD_CH * GramTile32::FS + 2 * IRLS_QUAD_CH + 2 * GramTile32::KP;
static_assert(IRLS_QUAD_WAVE_ELEMS == 64 * 36 + 2 * 64 + 2 * 32, "LDS layout of irls_nb_mfma32q_kernel");
template <int LT>
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void irls_nb_mfma32q_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols,
    const float* __restrict__ F, const float* __restrict__ Gbase, float* __restrict__ X, int k, float l1, float l2,
    int nonneg, int cd_maxit, int irls_max_iter, float irls_tol, const float* __restrict__ theta_row,
    const float* __restrict__ theta_col, int loss_type, float power, float robust,
    unsigned long long* __restrict__ stats) {
    constexpr int KP = GramTile32::KP, CH = IRLS_QUAD_CH, FS = GramTile32::FS;   // FS: also the stride of the G_w slab
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* Fst = reinterpret_cast<float*>(smem_raw) + (size_t)wave * IRLS_QUAD_WAVE_ELEMS;
    float2* sc = reinterpret_cast<float2*>(Fst + CH * FS);
    float* xs = Fst + CH * FS + 2 * CH;
    float* bws = xs + KP;
    float* Gl = Fst;                                    // [col][row], stride FS: reused once a column's Gram is complete
    const int64_t jw = ((int64_t)blockIdx.x * 4 + wave) * 4;      // first of this wave's four columns
    if (jw >= ncols) return;
    const int r = lane & 31, hh = lane >> 5;            // Gram phases: nonzero / feature r, half hh
    const int qme = lane >> 4, l = lane & 15;           // solve: column jw + qme, coordinates l and l + 16
    const int g8 = lane >> 3, p8 = lane & 7;            // gather: group of eight lanes = one row of F, lane = 16-byte piece
    const bool pok = 4 * p8 < k;
    const int64_t jme = jw + qme;
    const bool fok0 = l < k, fok1 = l + 16 < k;
    bool active = jme < ncols;                          // uniform over a row
    float x0 = 0.f, x1 = 0.f;                           // nnls_batch_irls.hpp:482-483  H.setZero(): no warm start
    int passes = 0, nsw = 0;      // IRLS passes; CD sweeps executed over all passes (work counters)
    float ng0[KP], ng1[KP];                             // rows l and l + 16 of the column's Gram, then of -G_w / G_ii
#pragma unroll
    for (int c = 0; c < KP; ++c) { ng0[c] = 0.f; ng1[c] = 0.f; }
    const float pinf = __builtin_inff();
    const float inf_rt = cd_maxit >= 0 ? pinf : 0.f;
    for (int irls = 0; irls < irls_max_iter; ++irls) {
        const unsigned long long act = __ballot(active);
        if (!act) break;
        if (active) ++passes;
        float b0 = 0.f, b1 = 0.f, gd0 = 0.f, gd1 = 0.f;
        for (int q = 0; q < 4; ++q) {
            if (!((act >> (16 * q)) & 1ull)) continue;                           // wave-uniform
            const int64_t j = jw + q;
            const int as = colptr[j], ae = colptr[j + 1];
            const float th_col = theta_col ? theta_col[j] : 0.f;
            if (qme == q) { xs[l] = x0; xs[l + 16] = x1; }
            GramTile32 tile(Fst, lane);
            tile.init_vec4(Gbase, k);
            float bw = 0.f;
            __builtin_amdgcn_wave_barrier();
            const float4 xq = *reinterpret_cast<const float4*>(xs + 4 * p8);    // the lane's piece of x
            for (int t0 = as; t0 < ae; t0 += CH) {
                // ---- phase A: lane t owns nonzero t of the chunk (its value, its weight); the gather is the group-of-eight form of
                // the kernel above with eight instructions, instruction i of group g taking chunk row 8g + i -- so lane t finds the
                // reconstruction of ITS nonzero in its own group at instruction t % 8, no shuffle
                const int tt = t0 + lane;
                const bool ok_me = tt < ae;
                const int row_me = ok_me ? rowidx[tt] : 0;
                const float a_me = ok_me ? vals[tt] : 0.f;
                float recon_me = 0.f;
                auto four_rows = [&](auto HC) {
                    constexpr int h4 = decltype(HC)::value;
                    float4 fv4[4];
                    cd_static_for<0, 4>([&](auto IC) {
                        constexpr int i = 4 * h4 + decltype(IC)::value;
                        const int rowg = (lane & 8) ? row_bcast_i<8 + i>(row_me) : row_bcast_i<i>(row_me);      // lane 8g + i of the wave
                        fv4[i - 4 * h4] = (t0 + 8 * g8 + i < ae && pok) ? *reinterpret_cast<const float4*>(F + (int64_t)rowg * k + 4 * p8)
                                                                       : make_float4(0.f, 0.f, 0.f, 0.f);
                    });
                    cd_static_for<0, 4>([&](auto IC) {
                        constexpr int u = decltype(IC)::value, i = 4 * h4 + u;
                        float part = fv4[u].x * xq.x;
                        part = tfma(fv4[u].y, xq.y, part);
                        part = tfma(fv4[u].z, xq.z, part);
                        part = tfma(fv4[u].w, xq.w, part);
                        part = sum8(part);                                           // W_T.col(row).dot(x), in the group's eight lanes
                        recon_me = p8 == i ? part : recon_me;
                        *reinterpret_cast<float4*>(Fst + (8 * g8 + i) * FS + 4 * p8) = fv4[u];
                    });
                };
                four_rows(std::integral_constant<int, 0>{});
                __builtin_amdgcn_sched_barrier(0);                                   // two batches of four loads: 16 registers, not 32
                four_rows(std::integral_constant<int, 1>{});
                const float th = theta_col ? th_col : (theta_row ? theta_row[row_me] : 0.f);
                const float w = irls_weight_full_dev<float>(LT >= 0 ? LT : loss_type, a_me - recon_me, recon_me, th, power, LT >= 0 ? 0.f : robust);
                sc[lane] = make_float2(ok_me ? w - 1.f : 0.f, ok_me ? w * a_me : 0.f);
                __builtin_amdgcn_wave_barrier();
                tile.update_staged(ae - t0 < CH ? ae - t0 : CH, sc, bw);     // phase B
                __builtin_amdgcn_wave_barrier();
            }
            bw += __shfl_xor(bw, 32, 64);
            // park G_w in the slab column by column ([col r][row gi], as the kernel above) and b_w next to it
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const int gi0 = 8 * v4 + 4 * hh;
                float4 val = make_float4(tile.acc[4 * v4], tile.acc[4 * v4 + 1], tile.acc[4 * v4 + 2], tile.acc[4 * v4 + 3]);
                if (l2 > 0.f && r < k) {
                    if (gi0 + 0 == r) val.x += l2;
                    if (gi0 + 1 == r) val.y += l2;
                    if (gi0 + 2 == r) val.z += l2;
                    if (gi0 + 3 == r) val.w += l2;
                }
                *reinterpret_cast<float4*>(Gl + r * FS + gi0) = val;
            }
            if (lane < KP) bws[lane] = bw;
            __builtin_amdgcn_wave_barrier();
            if (qme == q) {                              // the column's row picks up COLUMNS l and l + 16 of G_w
                // (columns, as the one-column kernel reads them: the MFMA's G_w(i, j) = sum ((w-1) f_i) f_j is not bitwise symmetric)
#pragma unroll
                for (int c4 = 0; c4 < KP / 4; ++c4) {
                    const float4 u = *reinterpret_cast<const float4*>(Gl + l * FS + 4 * c4);
                    const float4 v = *reinterpret_cast<const float4*>(Gl + (l + 16) * FS + 4 * c4);
                    ng0[4 * c4] = u.x; ng0[4 * c4 + 1] = u.y; ng0[4 * c4 + 2] = u.z; ng0[4 * c4 + 3] = u.w;
                    ng1[4 * c4] = v.x; ng1[4 * c4 + 1] = v.y; ng1[4 * c4 + 2] = v.z; ng1[4 * c4 + 3] = v.w;
                }
                gd0 = Gl[l * FS + l];
                gd1 = Gl[(l + 16) * FS + l + 16];
                b0 = bws[l];
                b1 = bws[l + 16];
            }
            __builtin_amdgcn_wave_barrier();
        }
        // ---- all (still iterating) columns of the wave at once: residual b_c = b_w - G_w x_old, coordinates in order
        const float xo0 = x0, xo1 = x1;
        {
            const float nx0 = -xo0, nx1 = -xo1;          // fma(-g, x, b) = fma(g, -x, b)
            cd_static_for<0, 16>([&](auto IC) { constexpr int i = decltype(IC)::value; row_fmac2<i>(b0, b1, nx0, ng0[i], ng1[i]); });
            cd_static_for<0, 16>([&](auto IC) { constexpr int i = decltype(IC)::value; row_fmac2<i>(b0, b1, nx1, ng0[16 + i], ng1[16 + i]); });
        }
        // cd_nnls_col_fixed(G_w, b_c, x, L1 inside, L2 = 0, nonneg, cd_maxit, ub = 0, tol = 0), static scaled form (kernels.hip.h):
        // d = b / G_ii - L1, rows scaled by -1 / G_ii once; a row that is done (or dead) holds zeros and never moves
        const bool alive0 = active && fok0 && gd0 > 0.f, alive1 = active && fok1 && gd1 > 0.f;
        const float ginv0 = alive0 ? 1.f / gd0 : 0.f, ginv1 = alive1 ? 1.f / gd1 : 0.f;
#pragma unroll
        for (int c = 0; c < KP; ++c) { ng0[c] *= -ginv0; ng1[c] *= -ginv1; }
        float d0 = __builtin_fmaf(active ? b0 : 0.f, ginv0, alive0 ? -l1 : 0.f);
        float d1 = __builtin_fmaf(active ? b1 : 0.f, ginv1, alive1 ? -l1 : 0.f);
        unsigned long long lane0_of_rows = 0x0001000100010001ull;
        asm volatile("" : "+s"(lane0_of_rows));        // opaque: shifted at run time, not sixteen 64-bit literals
        bool rowdone = !active;                          // (work counter: a row's sweeps until its own fixed point)
        for (int it = 0; it < cd_maxit; ++it) {
            nsw += rowdone ? 0 : 1;
            const float xe0 = nonneg ? x0 : pinf, xe1 = nonneg ? x1 : pinf;
            float aown0 = 0.f, aown1 = 0.f;
            const float nxe0 = -xe0, nxe1 = -xe1;
            // the lane whose turn it is keeps its step: lane mask of (l == i) as ONE scalar pair shifted by a SALU operation per
            // coordinate (sixteen compare results held in SGPRs cost 32 of them and spill)
            // Four VALU operations per coordinate and no wait state: the fmac of the OTHER residual is the previous coordinate's
            // (it is not on this half's chain) and sits, with the select, between the med3 that writes the step and the DPP read of it.
            unsigned long long turn = lane0_of_rows;
            float adp = sweep_first<0>(d0, aown0, nxe0, inf_rt, turn, ng0[0]);
            cd_static_for<1, 16>([&](auto IC) {
                constexpr int i = decltype(IC)::value;
                turn <<= 1;
                adp = sweep_step<i>(d0, d1, aown0, adp, nxe0, inf_rt, turn, ng0[i], ng1[i - 1]);
            });
            row_fmac1<15>(d1, adp, ng1[15]);
            turn = lane0_of_rows;
            adp = sweep_first<0>(d1, aown1, nxe1, inf_rt, turn, ng1[16]);
            cd_static_for<1, 16>([&](auto IC) {
                constexpr int i = decltype(IC)::value;
                turn <<= 1;
                adp = sweep_step<i>(d1, d0, aown1, adp, nxe1, inf_rt, turn, ng1[16 + i], ng0[16 + i - 1]);
            });
            row_fmac1<15>(d0, adp, ng0[31]);
            const float xn0 = x0 + aown0, xn1 = x1 + aown1;
            const bool moved = xn0 != x0 || xn1 != x1;
            x0 = xn0; x1 = xn1;
            const unsigned long long mv = __ballot(moved);
            if (!mv) break;
            // a column none of whose coordinates moved is at the fixed point the one-column kernel stops at: zero residuals make
            // every later step of its row exactly zero (the columns sharing the wave may need more sweeps)
            if (!((mv >> (lane & 48)) & 0xffffull)) { d0 = 0.f; d1 = 0.f; rowdone = true; }
        }
        float rel = fok0 ? tabs(x0 - xo0) / (tabs(xo0) + 1e-12f) : 0.f;
        const float rel1 = fok1 ? tabs(x1 - xo1) / (tabs(xo1) + 1e-12f) : 0.f;
        rel = rel1 > rel ? rel1 : rel;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const float o = __shfl_xor(rel, off, 64);
            rel = o > rel ? o : rel;
        }
        if (rel < irls_tol) active = false;
        __builtin_amdgcn_wave_barrier();
    }
    if (jme < ncols) {
        if (fok0) X[jme * (int64_t)k + l] = x0;
        if (fok1) X[jme * (int64_t)k + l + 16] = x1;
        // work counters (RCPPML_OPT_CD_COUNT_NOOP only): IRLS passes and nonzero-passes = weighted-Gram rank-1 updates
        if (stats && l == 0) {
            const int nzc = colptr[jme + 1] - colptr[jme];
            atomicAdd(stats, (unsigned long long)passes);
            atomicAdd(stats + 1, (unsigned long long)passes * (unsigned long long)nzc);
            atomicAdd(stats + 4, (unsigned long long)nsw);
        }
    }
}

// ---------------------------------------------------------------------------
// fp32, 32 < k <= 64 (k % 4 == 0): the same on a 2 x 2 grid of 32 x 32 accumulator tiles (the lower-left tile is the
// transpose of the upper-right one and is never computed: three MFMAs per pair of nonzeros).  Lane = feature in the sweep
// (all 64 lanes busy); in phase A a lane takes nonzero r and the 32 features of half hh (eight 16-byte gathers, the
// reconstruction f . x as 32 in-lane fmas + one half swap).  16 KiB of LDS per wave for G_w (the staged rows alias it):
// two blocks per CU -- an order of magnitude above the row-in-registers form this rank range used before (64 shuffles +
// 64 fmas per nonzero and lane), not the occupancy of the k <= 32 kernel.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void irls_nb_mfma32x2_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const float* __restrict__ vals, int64_t ncols,
    const float* __restrict__ F, const float* __restrict__ Gbase, float* __restrict__ X, int k, float l1, float l2,
    int nonneg, int cd_maxit, int irls_max_iter, float irls_tol, const float* __restrict__ theta_row,
    const float* __restrict__ theta_col, int loss_type, float power, float robust,
    unsigned long long* __restrict__ stats) {
    constexpr int CH = GramTile32x2::CH, FS = GramTile32x2::FS;   // FS: padded stride of a staged F row (64 features + bank spread)
    constexpr int GW = GramTile32x2::tile_elems;       // G_w slab; the staged rows (CH * FS = 2176 floats) alias its head
    constexpr int WAVE_FLOATS = irls_wave_elems<GramTile32x2>;   // G_w | (w-1, w a) pairs | x
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* Gl = reinterpret_cast<float*>(smem_raw) + (size_t)wave * WAVE_FLOATS;   // [c][r]
    float* Fst = Gl;
    float2* sc = reinterpret_cast<float2*>(Gl + GW);
    float* xs = Gl + GW + 2 * CH;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const int r = lane & 31, hh = lane >> 5;            // phase A: nonzero r, feature half hh; phase B: feature r (+32), K-slot hh
    const bool fok = lane < k;
    const int as = colptr[j], ae = colptr[j + 1];
    const float th_col = theta_col ? theta_col[j] : 0.f;
    float x = 0.f;                                      // nnls_batch_irls.hpp:482-483  H.setZero(): no warm start
    int passes = 0, nsw = 0;      // IRLS passes; CD sweeps executed over all passes (work counters)
    for (int irls = 0; irls < irls_max_iter; ++irls) {
        ++passes;
        GramTile32x2 tile(Gl, lane);                    // accumulator tiles <- base Gram
        tile.init(Gbase, k);
        xs[lane] = x;
        float bw0 = 0.f, bw1 = 0.f;                     // b_w of feature r and of feature 32 + r (this lane's K-slot share)
        __builtin_amdgcn_wave_barrier();
        for (int t0 = as; t0 < ae; t0 += CH) {
            // ---- phase A
            const int tt = t0 + r;
            const bool ok = tt < ae;
            const int row = ok ? rowidx[tt] : 0;
            const float a = ok ? vals[tt] : 0.f;
            const float* fsrc = F + (int64_t)row * k + 32 * hh;
            float4 fv4[8];
            float part = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c0 = 32 * hh + 4 * q;
                fv4[q] = (ok && c0 < k) ? *reinterpret_cast<const float4*>(fsrc + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 xv = *reinterpret_cast<const float4*>(xs + c0);
                part = tfma(fv4[q].x, xv.x, part);
                part = tfma(fv4[q].y, xv.y, part);
                part = tfma(fv4[q].z, xv.z, part);
                part = tfma(fv4[q].w, xv.w, part);
            }
            const float recon = part + __shfl_xor(part, 32, 64);                 // W_T.col(row).dot(x)
            const float th = theta_col ? th_col : (theta_row ? theta_row[row] : 0.f);
            const float w = irls_weight_full_dev<float>(loss_type, a - recon, recon, th, power, robust);
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<float4*>(Fst + r * FS + 32 * hh + 4 * q) = fv4[q];
            if (hh == 0) sc[r] = make_float2(ok ? w - 1.f : 0.f, ok ? w * a : 0.f);
            __builtin_amdgcn_wave_barrier();
            // ---- phase B
            tile.update(ae - t0 < CH ? ae - t0 : CH, [&](int t, const float (&f)[2]) {
                const float2 ws = sc[t];
                bw0 = tfma(ws.y, f[0], bw0);                                      // b_w += f * (w a)
                bw1 = tfma(ws.y, f[1], bw1);
                return ws.x;                                                      // G_w += (f (w-1)) f^T
            });
            __builtin_amdgcn_wave_barrier();
        }
        bw0 += __shfl_xor(bw0, 32, 64);
        bw1 += __shfl_xor(bw1, 32, 64);
        const float bw = hh ? bw1 : bw0;                 // lane = feature from here on
        tile.park(Gl, l2, k);
        __builtin_amdgcn_wave_barrier();
        // residual b_c = b_w - G_w x_old; the lane keeps its column of G_w in registers for the sweep
        const float x_old = x;
        float b = bw;
        nsw += tile.solve_cd<true>(Gl, b, x, fok, l1, nonneg, cd_maxit);
        float rel = fok ? tabs(x - x_old) / (tabs(x_old) + 1e-12f) : 0.f;
        rel = wave_max(rel);
        __builtin_amdgcn_wave_barrier();
        if (rel < irls_tol) break;
    }
    if (fok) X[j * (int64_t)k + lane] = x;
    // work counters (RCPPML_OPT_CD_COUNT_NOOP only): IRLS passes and nonzero-passes = weighted-Gram rank-1 updates
    if (stats && lane == 0) { atomicAdd(stats, (unsigned long long)passes); atomicAdd(stats + 1, (unsigned long long)passes * (unsigned long long)(ae - as)); atomicAdd(stats + 4, (unsigned long long)nsw); }
}

// ---------------------------------------------------------------------------
// fp64, k <= 32 (k % 2 == 0): the same kernel on v_mfma_f64_16x16x4_f64 -- the 32 x 32 weighted Gram is 2 x 2 tiles of
// 16 x 16, FOUR nonzeros fill the four K-slots of an instruction (A operand = (w_t - 1) f_t[16 ti + r], B operand =
// f_t[16 tj + r], lane (r = lane&15, kk = lane>>4) serves nonzero 4s + kk), C/D map col = lane&15, row = (lane>>4) + 4v.
// Phase A / CD solve as in irls_nb_mfma32_kernel (16-byte gathers = 2 doubles).
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void irls_nb_mfma64_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const double* __restrict__ vals, int64_t ncols,
    const double* __restrict__ F, const double* __restrict__ Gbase, double* __restrict__ X, int k, double l1, double l2,
    int nonneg, int cd_maxit, int irls_max_iter, double irls_tol, const double* __restrict__ theta_row,
    const double* __restrict__ theta_col, int loss_type, double power, double robust,
    unsigned long long* __restrict__ stats) {
    constexpr int KP = GramTile64::KP, CH = GramTile64::CH, FS = GramTile64::FS;   // FS: padded row stride (doubles) of the staged F rows
    constexpr int WAVE_DOUBLES = irls_wave_elems<GramTile64>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* Fst = reinterpret_cast<double*>(smem_raw) + (size_t)wave * WAVE_DOUBLES;
    double2* sc = reinterpret_cast<double2*>(Fst + CH * FS);
    double* xs = Fst + CH * FS + 2 * CH;
    double* Gl = Fst;                                   // [c][r], KP*KP <= CH*FS
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= ncols) return;
    const int r = lane & 31, hh = lane >> 5;            // phase A: nonzero r, feature half hh
    const bool fok = lane < k;
    const bool lin = lane < KP;
    const int as = colptr[j], ae = colptr[j + 1];
    const double th_col = theta_col ? theta_col[j] : 0.0;
    double x = 0.0;
    int passes = 0, nsw = 0;      // IRLS passes; CD sweeps executed over all passes (work counters)
    for (int irls = 0; irls < irls_max_iter; ++irls) {
        ++passes;
        GramTile64 tile(Fst, lane);
        tile.init(Gbase, k);
        if (lin) xs[lane] = x;
        double bw[2] = {0.0, 0.0};
        for (int t0 = as; t0 < ae; t0 += CH) {
            // ---- phase A
            const int tt = t0 + r;
            const bool ok = tt < ae;
            const int row = ok ? rowidx[tt] : 0;
            const double a = ok ? vals[tt] : 0.0;
            const double* fsrc = F + (int64_t)row * k + 16 * hh;
            double2 fv2[8];
            double part = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c0 = 16 * hh + 2 * q;
                fv2[q] = (ok && c0 < k) ? *reinterpret_cast<const double2*>(fsrc + 2 * q) : make_double2(0.0, 0.0);
                const double2 xv = *reinterpret_cast<const double2*>(xs + c0);
                part = tfma(fv2[q].x, xv.x, part);
                part = tfma(fv2[q].y, xv.y, part);
            }
            const double recon = part + __shfl_xor(part, 32, 64);
            const double th = theta_col ? th_col : (theta_row ? theta_row[row] : 0.0);
            const double w = irls_weight_full_dev<double>(loss_type, a - recon, recon, th, power, robust);
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<double2*>(Fst + r * FS + 16 * hh + 2 * q) = fv2[q];
            if (hh == 0) sc[r] = make_double2(ok ? w - 1.0 : 0.0, ok ? w * a : 0.0);
            __builtin_amdgcn_wave_barrier();
            // ---- phase B
            tile.update(ae - t0 < CH ? ae - t0 : CH, [&](int t, const double (&f)[2]) {
                const double2 ws = sc[t];
                bw[0] = tfma(ws.y, f[0], bw[0]);
                bw[1] = tfma(ws.y, f[1], bw[1]);
                return ws.x;
            });
            __builtin_amdgcn_wave_barrier();
        }
        // b_w[16 ti + r16]: sum over the four K-slot groups, then gather both halves into lane = feature order
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            bw[ti] += __shfl_xor(bw[ti], 16, 64);
            bw[ti] += __shfl_xor(bw[ti], 32, 64);
        }
        const double bwt = (lane & 16) ? bw[1] : bw[0];     // own registers: lane l < 32 has r16 = l & 15 and wants feature l
        tile.park(Gl, l2, k);
        __builtin_amdgcn_wave_barrier();
        const double x_old = x;
        double b = bwt;
        nsw += tile.solve_cd<true>(Gl, b, x, fok, l1, nonneg, cd_maxit);
        double rel = fok ? tabs(x - x_old) / (tabs(x_old) + 1e-12) : 0.0;
        rel = wave_max(rel);
        __builtin_amdgcn_wave_barrier();
        if (rel < irls_tol) break;
    }
    if (fok) X[j * (int64_t)k + lane] = x;
    // work counters (RCPPML_OPT_CD_COUNT_NOOP only): IRLS passes and nonzero-passes = weighted-Gram rank-1 updates
    if (stats && lane == 0) { atomicAdd(stats, (unsigned long long)passes); atomicAdd(stats + 1, (unsigned long long)passes * (unsigned long long)(ae - as)); atomicAdd(stats + 4, (unsigned long long)nsw); }
}

}  // namespace rk
