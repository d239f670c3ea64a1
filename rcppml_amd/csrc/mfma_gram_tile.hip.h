// ============================================================================
// mfma_gram_tile.hip.h -- a per-column k x k Gram held in the MFMA accumulators of ONE wavefront, for the kernels that correct
// the shared Gram column by column: the IRLS half-update (kernels_irls.hip.h: G_w = G + sum (w - 1) f f^T) and the
// cross-validation half-update (kernels_cv.hip.h: G_local = G - sum over held-out rows f f^T).
//
// A tile policy owns the accumulators and says how they meet LDS.  Life of a tile, per column (IRLS: per pass):
//   init(G, k)          accumulators <- base Gram, identity beyond k, through the instruction's C/D map
//                         fp32 32x32x2:  col = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
//                         fp64 16x16x4:  col = lane & 15, row = (lane >> 4) + 4 v
//   [caller]            parks up to CH rows of F in the staging area Fst (row stride FS: bank spread); rows it does not
//                       have are parked as ZERO rows, so a count rounded up to a whole MFMA step adds exact zeros
//   update(cnt, scale)  (2 x 2 tiles; IRLS) rank-cnt update from the staged rows: two (fp32) or four (fp64) rows fill the K-slots
//                       of one MFMA step, A operand = scale(t, f) * f, B operand = f; one conflict-free LDS read of f_t[r] per
//                       lane feeds both operands.  The caller's `scale` hands back the staged weight w_t - 1 and accumulates
//                       the right-hand side b_w += w_t a_t f_t from the same f on the way.
//   update_staged       (32 x 32 tile; IRLS) the same with the pairs read by the tile, four steps' LDS reads ahead of their MFMAs
//   flush(cnt, hq, F, k)  (CV) gathers cnt <= 32 queued rows of F into the staging area itself (lane = row, feature half) and
//                       applies G -= f f^T: A operand = -f
//   park(Gl, l2, k)     the tile to LDS as [c][r] (+ l2 on the diagonal below k); Gl aliases the staging area
//   solve_cd<RESID>     the lane picks up ITS column of the parked Gram (RESID: forming b -= G x on the way, the
//                       warm-start residual) and runs the static coordinate sweeps of kernels.hip.h; returns the sweeps
// Constants: Scalar, Pair (the staged (w - 1, w a) pair), KP (padded rank), FS, CH (rows per chunk), NF (features a lane
// serves in update), tile_elems (LDS elements of staging area / parked Gram).  What a kernel puts behind the tile (IRLS: the
// pairs and x; CV: its row queue) is the kernel's; its element count stands next to the kernel and the host sizes the launch
// from that constant.
// The pass loops stay with the kernels, and irls_nb_mfma32_kernel (64 VGPRs) also keeps its own park and column pickup: its
// register allocation does not survive a frame shared with the other tiles (docs/kernel_notes.md).  flush keeps each tile's own
// gather and loop: the CV kernels compile to the code they had with their private tiles.
// ============================================================================
#pragma once
#include "kernels.hip.h"

namespace rk {

typedef float f32x32 __attribute__((ext_vector_type(32)));

// fp32, k <= 32 (k % 4 == 0): one 32 x 32 tile, v_mfma_f32_32x32x2_f32; update: feature r, K-slot hh
struct GramTile32 {
    typedef float Scalar;
    typedef float2 Pair;
    static constexpr int KP = 32, FS = 36, CH = 32, NF = 1;
    static constexpr int tile_elems = CH * FS;        // KP * KP <= CH * FS: the parked Gram fits the staging area
    float* Fst;
    int lane, r, hh;
    f32x16 acc;
    __device__ __forceinline__ GramTile32(float* st, int lane_) : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5) {}
    __device__ __forceinline__ void init(const float* __restrict__ G, int k) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh, gj = r;
            acc[v] = (gi < k && gj < k) ? G[(int64_t)gj * k + gi] : (gi == gj ? 1.f : 0.f);
        }
    }
    // the same with four 16-byte loads off one per-lane pointer (the Gram is symmetric: column r read as row r), for callers
    // that have G 16-byte aligned; k % 4 == 0 keeps a group of four rows on one side of k
    __device__ __forceinline__ void init_vec4(const float* __restrict__ G, int k) {
        const float* gb = G + (int64_t)r * k + 4 * hh;
        asm volatile("" : "+v"(gb));                 // formed where it is used, not 16 hoisted addresses
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {
            const int gi0 = 8 * v4 + 4 * hh;
            const float4 g = (gi0 < k && r < k) ? *reinterpret_cast<const float4*>(gb + 8 * v4) : make_float4(0.f, 0.f, 0.f, 0.f);
            const bool pad = r >= k;
            acc[4 * v4 + 0] = pad && gi0 + 0 == r ? 1.f : g.x;
            acc[4 * v4 + 1] = pad && gi0 + 1 == r ? 1.f : g.y;
            acc[4 * v4 + 2] = pad && gi0 + 2 == r ? 1.f : g.z;
            acc[4 * v4 + 3] = pad && gi0 + 3 == r ? 1.f : g.w;
        }
    }
    // CV: gather the first cnt <= 32 queued rows (lane = row t, feature half hh) and apply G -= f f^T
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
    // update with scale = sc[t].x and bw += sc[t].y f, in groups of four steps: the eight LDS reads of a group are issued
    // ahead of its MFMAs (the count is rounded up to a whole group: zero rows with zero pairs)
    __device__ __forceinline__ void update_staged(int cnt, const float2* sc, float& bw) {
        const int nst = (cnt + 1) >> 1;
        for (int s2 = 0; s2 < nst; s2 += 4) {
            float fv[4];
            float2 ws[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = 2 * (s2 + u) + hh;
                fv[u] = Fst[t * FS + r];
                ws[u] = sc[t];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bw = tfma(ws[u].y, fv[u], bw);                                    // b_w += f * (w a)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ws[u].x * fv[u], fv[u], acc, 0, 0, 0);   // G_w += (f (w-1)) f^T
            }
        }
    }
    // (symmetric, so accumulator row i is written as slab row i)
    __device__ __forceinline__ void park(float* Gl, float l2, int k) const {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh;
            float val = acc[v];
            if (l2 > 0.f && gi == r && gi < k) val += l2;
            Gl[gi * KP + r] = val;
        }
    }
    // The lane keeps ITS column of the Gram -- G(c, ll), c = 0..31 -- in registers: the sweep picks row i of it with a
    // wave-uniform index, i.e. a register-indexed move instead of an LDS read on the dependent chain of every step.
    template <bool RESID>
    __device__ __forceinline__ int solve_cd(const float* Gl, float& b, float& x, bool fok, float l1, int nonneg, int maxit) const {
        static_assert(!RESID, "irls_nb_mfma32_kernel forms its residual itself");
        const int ll = lane < KP ? lane : 0;
        const float gd = Gl[ll * KP + ll];
        f32x32 gcol;
#pragma unroll
        for (int c = 0; c < KP; ++c) gcol[c] = Gl[c * KP + ll];
        float gg[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) gg[c] = gcol[c];
        return cd_static_sweeps_scaled_f32<KP>(b, x, gd, fok, l1, nonneg, maxit, gg);
    }
};

// fp32, 32 < k <= 64 (k % 4 == 0): a 2 x 2 grid of 32 x 32 tiles (three MFMAs per pair of rows; the lower-left tile is the
// transpose of the upper-right one and is never computed), lane = feature over the whole wave in the solve; 16 KiB of LDS per
// wave for the parked Gram, whose head doubles as the 32 x FS staging area (two blocks per CU)
struct GramTile32x2 {
    typedef float Scalar;
    typedef float2 Pair;
    static constexpr int KP = 64, FS = 68, CH = 32, NF = 2;
    static constexpr int tile_elems = KP * KP;
    float* Fst;
    int lane, r, hh;
    f32x16 a00, a01, a11;                             // rows 0-31 x cols 0-31 | rows 0-31 x cols 32-63 | rows 32-63 x cols 32-63
    __device__ __forceinline__ GramTile32x2(float* st, int lane_) : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5) {}
    __device__ __forceinline__ void init(const float* __restrict__ G, int k) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh, gj = r;
            auto base = [&](int i2, int j2) { return (i2 < k && j2 < k) ? G[(int64_t)j2 * k + i2] : (i2 == j2 ? 1.f : 0.f); };
            a00[v] = base(gi, gj); a01[v] = base(gi, gj + 32); a11[v] = base(gi + 32, gj + 32);
        }
    }
    // CV: as GramTile32::flush
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
    template <class S> __device__ __forceinline__ void update(int cnt, S&& scale) {
        const int nst = (cnt + 1) >> 1;
#pragma unroll 2
        for (int s2 = 0; s2 < nst; ++s2) {
            const int t = 2 * s2 + hh;
            const float f[2] = {Fst[t * FS + r], Fst[t * FS + 32 + r]};
            const float s = scale(t, f);
            const float s0 = s * f[0], s1 = s * f[1];
            a00 = __builtin_amdgcn_mfma_f32_32x32x2f32(s0, f[0], a00, 0, 0, 0);
            a01 = __builtin_amdgcn_mfma_f32_32x32x2f32(s0, f[1], a01, 0, 0, 0);
            a11 = __builtin_amdgcn_mfma_f32_32x32x2f32(s1, f[1], a11, 0, 0, 0);
        }
    }
    __device__ __forceinline__ void park(float* Gl, float l2, int k) const {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int gi = (v & 3) + 8 * (v >> 2) + 4 * hh;      // row inside the tile; column inside the tile = r
            float d00 = a00[v], d11 = a11[v];
            if (l2 > 0.f && gi == r) { if (gi < k) d00 += l2; if (gi + 32 < k) d11 += l2; }
            Gl[gi * KP + r] = d00;                               // symmetric tile: stored as computed
            Gl[gi * KP + 32 + r] = a01[v];                       // G(row 32 + r, col gi) at [c = gi][r' = 32 + r] (next to d00: one paired write)
            Gl[(32 + r) * KP + gi] = a01[v];                     // and its mirror G(row gi, col 32 + r) at [c = 32 + r][r' = gi]
            Gl[(gi + 32) * KP + 32 + r] = d11;
        }
    }
    // as GramTile32::solve_cd, the column in two halves: hipcc indexes 32-element vectors with s_set_gpr_idx, 64-element ones
    // through scratch
    template <bool RESID>
    __device__ __forceinline__ int solve_cd(const float* Gl, float& b, float& x, bool fok, float l1, int nonneg, int maxit) const {
        float gd;
        f32x32 gcol0, gcol1;
        if constexpr (RESID) {                        // b -= G x in coordinate order: first half, then second
            const float x_old = x;
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const float gv = Gl[c * KP + lane];
                gcol0[c] = gv;
                b = tfma(-gv, __shfl(x_old, c, 64), b);
            }
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const float gv = Gl[(32 + c) * KP + lane];
                gcol1[c] = gv;
                b = tfma(-gv, __shfl(x_old, 32 + c, 64), b);
            }
            gd = Gl[lane * KP + lane];
        } else {
            gd = Gl[lane * KP + lane];
#pragma unroll
            for (int c = 0; c < 32; ++c) { gcol0[c] = Gl[c * KP + lane]; gcol1[c] = Gl[(32 + c) * KP + lane]; }
        }
        float gg[KP];
#pragma unroll
        for (int c = 0; c < 32; ++c) { gg[c] = gcol0[c]; gg[32 + c] = gcol1[c]; }
        return cd_static_sweeps_scaled_f32<KP>(b, x, gd, fok, l1, nonneg, maxit, gg);
    }
};

// fp64, k <= 32 (k % 2 == 0): 2 x 2 tiles of 16 x 16, v_mfma_f64_16x16x4_f64 (four rows per instruction step); update: feature
// slot r16 (features r16 and 16 + r16), K-slot kk
struct GramTile64 {
    typedef double Scalar;
    typedef double2 Pair;
    static constexpr int KP = 32, FS = 34, CH = 32, NF = 2;
    static constexpr int tile_elems = CH * FS;        // KP * KP <= CH * FS
    double* Fst;
    int lane, r, hh, r16, kk;                         // staging: row r, half hh
    f64x4 acc[2][2];
    __device__ __forceinline__ GramTile64(double* st, int lane_)
        : Fst(st), lane(lane_), r(lane_ & 31), hh(lane_ >> 5), r16(lane_ & 15), kk(lane_ >> 4) {}
    __device__ __forceinline__ void init(const double* __restrict__ G, int k) {
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int gi = 16 * ti + kk + 4 * v, gj = 16 * tj + r16;
                    acc[ti][tj][v] = (gi < k && gj < k) ? G[(int64_t)gj * k + gi] : (gi == gj ? 1.0 : 0.0);
                }
    }
    // CV: as GramTile32::flush
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
    template <class S> __device__ __forceinline__ void update(int cnt, S&& scale) {
        const int nst = (cnt + 3) >> 2;
#pragma unroll 2
        for (int s4 = 0; s4 < nst; ++s4) {
            const int t = 4 * s4 + kk;
            const double f[2] = {Fst[t * FS + r16], Fst[t * FS + 16 + r16]};
            const double s = scale(t, f);
            const double a0 = s * f[0], a1 = s * f[1];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, f[0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, f[1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, f[0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, f[1], acc[1][1], 0, 0, 0);
        }
    }
    __device__ __forceinline__ void park(double* Gl, double l2, int k) const {
        double* const g0 = Gl + kk * KP + r16;          // one base, compile-time offsets
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int gi = 16 * ti + kk + 4 * v, gj = 16 * tj + r16;
                    double val = acc[ti][tj][v];
                    if (l2 > 0.0 && gi == gj && gi < k) val += l2;
                    g0[(16 * ti + 4 * v) * KP + 16 * tj] = val;
                }
    }
    // the lane's Gram column read from the wave's LDS tile at compile-time offsets (cd_static_sweeps, kernels.hip.h)
    template <bool RESID>
    __device__ __forceinline__ int solve_cd(const double* Gl, double& b, double& x, bool fok, double l1, int nonneg, int maxit) const {
        const int ll = lane < KP ? lane : 0;
        if constexpr (RESID) {
            const double x_old = x;
#pragma unroll 8
            for (int c = 0; c < KP; ++c) b = tfma(-Gl[c * KP + ll], __shfl(x_old, c, 64), b);
        }
        const double gd = Gl[ll * KP + ll];
        return cd_static_sweeps<double, KP>(b, x, gd, fok, l1, nonneg, maxit, [&](auto IC) { return Gl[decltype(IC)::value * KP + ll]; });
    }
};

}  // namespace rk
