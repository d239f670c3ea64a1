// kernels_stream_svd.hip.h -- the block products of a panel-streamed randomized SVD (ops_stream_svd.hip).  The
// matrix passes through the device one column panel at a time and its transpose is never built, so the product in the scatter
// direction, Y = A~ X (l x m from l x n), comes from a panel's column form:
//   stream_block_scatter_kernel  Y[:, r] (+)= sum_{j in panel} a_rj X[:, j], accumulators in registers
//   stream_block_finish_kernel   after the last panel of a pass: the centering term and the block's records
//   stream_fill_kernel / stream_scale_kernel  the ones and the 1 / n of the row-mean pass (the scatter kernel at l = 1)
// The gather direction is rs_prod_kernel (kernels_svd_rand.hip.h) on the panel's own column pointers.
//
// Work split.  A wavefront owns a slice of SB_RW = 8 rows per lane group; a workgroup is four such wavefronts and nothing more (no
// LDS, no barrier), so the tile is small: 32 rows for l > 32, and 13 714 rows give 1716 wavefronts, 6.7 per CU.  A lane is a
// component (two for 64 < l <= 128).  For l <= 32 the wavefront splits into NG = 64 / LP lane groups that own consecutive
// 8-row sub-slices, so one walk over the panel's columns (the range table, the prefetch) serves NG * 8 rows.
// Registers, not LDS: a nonzero's row is wave-uniform after the broadcast, so the accumulator is picked by a scalar compare and
// the dependent chain of one output element is one FMA (4 cycles), not an LDS read-modify-write (the chain 4.18 names); 8 rows x
// 2 components x fp64 are 32 VGPRs.
// In flight.  Lane j of a wavefront fetches the range of column j0 + j in the slice (stream_tile_ptr_kernel's table) and
// prefetches its first SB_P = 8 (row, value) pairs -- for l > 32 all a column can hold in the slice -- so the nonzeros of 64
// columns are loaded in eight independent rounds before any is consumed.  The live lanes are then taken in ascending column
// order, four at a time: the four columns of X are loaded first, then the broadcast nonzeros are applied.  Only for l <= 32, where
// a slice has 16 to 64 rows, can a column hold more than eight; the rest is read in place.
// Order.  An element of Y has one owner (slice, lane group, lane) and receives its additions in panel order, then ascending column
// (a column holds a row once), with no atomics: the result depends on the data and (dtype, l) only, not on the grid.
#pragma once
#include "kernels_stream.hip.h"
#include "kernels_svd_rand.hip.h"

namespace rstream_svd {
using namespace rsv;

constexpr int SB_RW = 8;                 // rows per lane group: the accumulators of a lane
constexpr int SB_U = 4;                  // live columns whose X loads are issued together
constexpr int SB_P = 8;                  // (row, value) pairs a lane prefetches of its column: all a column can hold in 8 rows

// lanes per l-vector: 8, 16, 32 or 64 (64 with two components per lane above 64)
inline int sb_lp(int l) { return l <= 8 ? 8 : l <= 16 ? 16 : l <= 32 ? 32 : 64; }
inline int sb_wave_rows(int l) { return SB_RW * (WAVE / sb_lp(l)); }      // rows of a wavefront's slice
inline int sb_tile_rows(int l) { return NW * sb_wave_rows(l); }           // rows of a workgroup

template <class T, int NC>
__device__ inline void sb_apply(T (&a0)[SB_RW], T (&a1)[SB_RW], int t, T v, T h0, T h1) {
#pragma unroll
    for (int u = 0; u < SB_RW; ++u)
        if (t == u) {                    // t is wave-uniform: a scalar branch picks the register
            a0[u] += v * h0;
            if (NC == 2) a1[u] += v * h1;
        }
}

// tp: the table of stream_tile_ptr_kernel for slices of RWV = SB_RW * (64 / LP) rows, nsl of them.  X: l x pc, Y: l x m.
template <class T, int LP, int NC>
__global__ __launch_bounds__(WG) void stream_block_scatter_kernel(const int* __restrict__ ri, const T* __restrict__ ax,
                                                                  const int* __restrict__ tp, int64_t pc, int64_t m, int64_t nsl,
                                                                  const T* __restrict__ X, int l, int accumulate, T* __restrict__ Y) {
    constexpr int NG = WAVE / LP, RWV = SB_RW * NG;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int c0 = lane % LP, g = lane / LP, c1 = c0 + WAVE;
    const bool on0 = c0 < l, on1 = NC == 2 && c1 < l;
    for (int64_t sl = (int64_t)blockIdx.x * NW + wave; sl < nsl; sl += (int64_t)gridDim.x * NW) {
        const int64_t row0 = sl * RWV, grow0 = row0 + (int64_t)g * SB_RW;
        T a0[SB_RW], a1[SB_RW];
#pragma unroll
        for (int u = 0; u < SB_RW; ++u) {
            const bool in = accumulate && grow0 + u < m;
            a0[u] = in && on0 ? Y[(grow0 + u) * l + c0] : T(0);
            a1[u] = in && on1 ? Y[(grow0 + u) * l + c1] : T(0);
        }
        const int* tb = tp + sl * pc;
        for (int64_t j0 = 0; j0 < pc; j0 += WAVE) {
            int s = 0, cnt = 0, rr[SB_P];
            T vv[SB_P];
            if (j0 + lane < pc) { s = tb[j0 + lane]; cnt = tb[pc + j0 + lane] - s; }
#pragma unroll
            for (int e = 0; e < SB_P; ++e) {
                rr[e] = e < cnt ? ri[s + e] : 0;
                vv[e] = e < cnt ? ax[s + e] : T(0);
            }
            unsigned long long live = __ballot(cnt > 0);
            while (live) {
                int cc[SB_U];
                T h0[SB_U], h1[SB_U];
#pragma unroll
                for (int u = 0; u < SB_U; ++u) {
                    cc[u] = live ? __ffsll((long long)live) - 1 : -1;
                    live &= live - 1;                           // 0 stays 0
                }
#pragma unroll
                for (int u = 0; u < SB_U; ++u) {
                    const T* x = X + (j0 + max(cc[u], 0)) * l;
                    h0[u] = cc[u] >= 0 && on0 ? x[c0] : T(0);
                    h1[u] = cc[u] >= 0 && on1 ? x[c1] : T(0);
                }
#pragma unroll
                for (int u = 0; u < SB_U; ++u) {
                    if (cc[u] < 0) break;
                    const int n_c = __shfl(cnt, cc[u]), s_c = __shfl(s, cc[u]);
#pragma unroll
                    for (int e = 0; e < SB_P; ++e) {
                        if (e >= n_c) break;
                        const int rl = __builtin_amdgcn_readfirstlane(__shfl(rr[e], cc[u]) - (int)row0);
                        const T v = __shfl(vv[e], cc[u]);
                        if ((unsigned)rl >= (unsigned)RWV) continue;        // the table keeps every entry inside the slice
                        if (g == rl / SB_RW) sb_apply<T, NC>(a0, a1, rl % SB_RW, v, h0[u], h1[u]);
                    }
                    for (int e = SB_P; e < n_c; ++e) {                      // only where a slice has more than SB_P rows (l <= 32)
                        const int rl = __builtin_amdgcn_readfirstlane(ri[s_c + e] - (int)row0);
                        const T v = ax[s_c + e];
                        if ((unsigned)rl >= (unsigned)RWV) continue;
                        if (g == rl / SB_RW) sb_apply<T, NC>(a0, a1, rl % SB_RW, v, h0[u], h1[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SB_RW; ++u) {
            if (grow0 + u >= m) break;
            if (on0) Y[(grow0 + u) * l + c0] = a0[u];
            if (on1) Y[(grow0 + u) * l + c1] = a1[u];
        }
    }
}

// After the last panel of a pass over X (l x len): center 1 subtracts mu[row] * cs and center 2 subtracts cs, cs being the column
// sums re-added from the nbin records Pin of the block that was multiplied (as rs_prod_kernel does per row); then the record of
// the workgroup's RS_RB rows, in the layout rs_chol_kernel and rs_apply_kernel read.
template <class T, int TI>
__global__ __launch_bounds__(WG) void stream_block_finish_kernel(T* X, long len, int l, const double* __restrict__ Pin, int nbin,
                                                                 const T* __restrict__ mu, int center, double* __restrict__ Pout) {
    __shared__ T xs[RS_GS * RS_LMAX];
    __shared__ double cs[RS_LMAX];
    const long b0 = (long)blockIdx.x * RS_RB, bend = min(len, b0 + RS_RB);
    if (center) {
        const int np = rs_np(l);
        for (int c = threadIdx.x; c < l; c += WG) cs[c] = rs_readd(Pin + l * l + c, nbin, np);
        __syncthreads();
        for (int e = threadIdx.x; e < (int)(bend - b0) * l; e += WG) {
            const long row = b0 + e / l;
            const T sc = (T)cs[e % l];
            X[row * l + e % l] -= center == 1 ? mu[row] * sc : sc;
        }
        __syncthreads();
    }
    rs_record<T, TI>(X, b0, bend, l, nullptr, 1, Pout + (long)blockIdx.x * rs_np(l), xs);
}

template <class T>
__global__ __launch_bounds__(WG) void stream_fill_kernel(T* __restrict__ v, int64_t count, T value) {
    const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (e < count) v[e] = value;
}
// v <- v / div: the row sums of the mean pass become the row means
template <class T>
__global__ __launch_bounds__(WG) void stream_scale_kernel(T* __restrict__ v, int64_t count, T div) {
    const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (e < count) v[e] = v[e] / div;
}

}  // namespace rstream_svd
