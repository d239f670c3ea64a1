// kernels_stream.hip.h -- the W-side sums of a panel-streamed fit (ops_stream.hip).  A streamed fit sees the matrix
// one column panel at a time and never builds its transpose, so the W half-update's right-hand side B_W = H A^T and Gram
// G_H = H H^T are accumulated panel by panel:
//   stream_tile_ptr_kernel   per panel visit: for every column of the panel, where the rows of each wave's row slice begin
//   stream_rhs_w_kernel      B_W[:, r] (+)= sum_{j in panel} a_rj H[:, j], straight from the panel's column form
//   stream_gram_add_kernel   G_acc (+)= the panel's Gram partial tiles (the MFMA kernels of kernels.hip.h), in tile order
//   stream_gram_finish_kernel  G = diag(1/d) G_acc diag(1/d) + eps I + l2 I once, after the last panel
//   stream_sum_kernel        ||A||^2 = the panels' sums of squares added in panel order
// No atomics anywhere: every output element has one owner and one order of additions, which depends on the data and on
// (dtype, k) only -- not on the grid.
#pragma once
#include "kernels.hip.h"

namespace rstream {

constexpr int NW = 4;                   // wavefronts per workgroup; each owns a contiguous slice of the tile's rows
constexpr int NT = 64 * NW;
constexpr int CB = 64;                  // columns of H_p staged in LDS at a time (one per lane of the pointer loads)
constexpr int ACC_BYTES = 32 * 1024;    // accumulator tile per workgroup

// padded rank: 8, 16, 32 or 64 lanes per k-vector
inline int k_pad(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
// rows of a tile: KP x R accumulators fill ACC_BYTES; a function of (dtype, k) only
inline int tile_rows(size_t elem, int k) { return (int)(ACC_BYTES / (k_pad(k) * elem)); }
template <class T, int KP> constexpr size_t lds_bytes() { return ACC_BYTES + (size_t)CB * KP * sizeof(T); }

// tp[b * pc + j] = the first nonzero of panel column j whose row is >= b * RW (b = 0 .. nb: wave slice boundaries; rows are
// sorted within a column, so slice b of column j is the contiguous range tp[b * pc + j] .. tp[(b + 1) * pc + j])
static __global__ __launch_bounds__(256) void stream_tile_ptr_kernel(const int* __restrict__ cp, const int* __restrict__ ri, int64_t pc,
                                                              int64_t nb, int RW, int* __restrict__ tp) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (nb + 1) * pc) return;
    const int64_t b = t / pc, j = t - b * pc;
    const int64_t row = b * RW;
    int lo = cp[j], hi = cp[j + 1];
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ri[mid] < row) lo = mid + 1; else hi = mid;
    }
    tp[t] = lo;
}

// One workgroup per row tile (grid-stride over the tiles), wave w owns rows [tile * R + w * RW, + RW).  The wave walks the panel's
// columns in ascending order, CB at a time: the CB columns of H_p are staged in LDS by the whole workgroup, lane l fetches the
// range of column l, and the non-empty ranges are visited in column order.  The wave is split into NG = 64 / KP lane groups that
// take consecutive nonzeros of one column: rows increase strictly within a column, so the groups of one step write different
// LDS columns, and every row receives its additions in ascending column order whichever group carries them.
template <class T, int KP>
__global__ __launch_bounds__(NT) void stream_rhs_w_kernel(const int* __restrict__ ri, const T* __restrict__ ax,
                                                          const int* __restrict__ tp, int64_t pc, int64_t m, int64_t ntiles,
                                                          const T* __restrict__ H, int k, int accumulate, T* __restrict__ BW) {
    constexpr int R = ACC_BYTES / (KP * (int)sizeof(T)), RW = R / NW, NG = 64 / KP;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* acc = reinterpret_cast<T*>(smem_raw);                   // [R][KP]
    T* hs = reinterpret_cast<T*>(smem_raw + ACC_BYTES);        // [CB][KP]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = lane & (KP - 1), g = lane / KP;
    T* wacc = acc + wave * RW * KP;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * R + (int64_t)wave * RW;
        const int64_t b = tile * NW + wave;
        // the wave's slice of the tile: zero on the first panel of a pass, else what the earlier panels left in B_W
        for (int r = g; r < RW; r += NG) {
            const int64_t row = row0 + r;
            wacc[r * KP + f] = (accumulate && row < m && f < k) ? BW[row * k + f] : T(0);
        }
        for (int64_t j0 = 0; j0 < pc; j0 += CB) {
            __syncthreads();                                   // the previous batch's readers are done with hs
            for (int e = threadIdx.x; e < CB * KP; e += NT) {
                const int c = e / KP, ff = e & (KP - 1);
                hs[e] = (j0 + c < pc && ff < k) ? H[(j0 + c) * k + ff] : T(0);
            }
            __syncthreads();
            int s = 0, en = 0;
            if (j0 + lane < pc) { s = tp[b * pc + j0 + lane]; en = tp[(b + 1) * pc + j0 + lane]; }
            unsigned long long live = __ballot(en > s);
            while (live) {
                const int c = __ffsll((long long)live) - 1;
                live &= live - 1;
                const int sc = __shfl(s, c, 64), ec = __shfl(en, c, 64);
                const T hv = hs[c * KP + f];
                for (int q = sc + g; q < ec; q += NG) {
                    const int r = ri[q] - (int)row0;
                    if ((unsigned)r < (unsigned)RW) wacc[r * KP + f] += ax[q] * hv;
                }
                __builtin_amdgcn_wave_barrier();               // the next column may reach these rows through another lane group
            }
        }
        for (int r = g; r < RW; r += NG) {
            const int64_t row = row0 + r;
            if (row < m && f < k) BW[row * k + f] = wacc[r * KP + f];
        }
        __syncthreads();                                       // hs is restaged by the next tile
    }
}

// G_acc (+)= the panel's partial tiles, added in tile order (one thread per element of the k x k result)
template <class T>
__global__ __launch_bounds__(256) void stream_gram_add_kernel(const T* __restrict__ partial, int nblk, int KP, int k, int accumulate,
                                                              T* __restrict__ Gacc) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k * k) return;
    const int i = e % k, j = e / k;
    T s = 0;
    for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * KP * KP + (int64_t)j * KP + i];
    Gacc[e] = accumulate ? Gacc[e] + s : s;
}

// the Gram of the SCALED factor from the sums of the unscaled one: G(i, j) = G_acc(i, j) / (d_i d_j), then eps and l2 on the
// diagonal in the order gram_finalize adds them.  d may be null (no scaling).
template <class T>
__global__ __launch_bounds__(256) void stream_gram_finish_kernel(const T* __restrict__ Gacc, const T* __restrict__ d, int k, T eps, T l2,
                                                                 T* __restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k * k) return;
    const int i = e % k, j = e / k;
    T s = Gacc[e];
    if (d) s = s / (d[i] * d[j]);
    if (i == j) { s += eps; s += l2; }
    G[e] = s;
}

// out[0] = v[0] + v[1] + ... in index order
static __global__ void stream_sum_kernel(const double* __restrict__ v, int count, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0;
    for (int q = 0; q < count; ++q) s += v[q];
    out[0] = s;
}

}  // namespace rstream
