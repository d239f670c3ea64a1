// kernels_graph.hip.h -- the two kernels a multi-layer factor graph needs beside the fit's own ops (ops_graph.hip), fp64.
//
// graph_assemble_kernel.  The effective input of a deeper layer (reference graph/fit.hpp:100-194): X (n x c, column-major) from up
// to GRAPH_MAX_BRANCHES upstream factors H_b (k_b x n, leading dimension k_b) and an optional condition block Z (p x n).
//   concat: X = [t(H_1) | t(H_2) | ... | t(Z)],  c = k_1 + k_2 + ... + p   (one branch: the plain chain X = t(H_up))
//   add:    X = [t(H_1 + H_2 + ...) | t(Z)],     c = k + p, summed in branch order
// A transposing gather through a TILE x TILE LDS tile: a workgroup reads TILE output columns (consecutive features of a branch:
// consecutive addresses) for TILE samples, and writes them with the sample index fastest (consecutive addresses of X).  The tile's
// rows are TILE + 1 doubles long: the column read of the write phase then touches every bank pair once per 32 lanes (ds_read_b64
// banks are (a / 4) mod 64; an even row length would put lanes l and l + 1 on the same pair).  No atomics: every output element is
// written once, by one thread, and add's sum runs in branch order in that thread.
//
// graph_layer_loss_kernel / graph_loss_final_kernel.  sum_ij (X_ij - sum_f W_T[f, i] d_f H[f, j])^2 for a dense X (rows x c,
// column-major), W_T k x rows, H k x c, k <= GRAPH_MAX_K.  One workgroup per LOSS_ROWS rows of X: it stages its W_T rows times d
// (one contiguous, coalesced read) and, LOSS_CT columns at a time, the columns of H in LDS; thread (row, column pair) forms its
// two products in registers, squares the differences and keeps one running sum over the column tiles.  The workgroup's NT sums go
// through a fixed-order tree into one partial.  graph_loss_final_kernel (one workgroup) adds the partials in index order per
// thread segment, then the same tree, scales and writes the layer's loss.  The chunking depends on (rows, c, k) only -- not on the
// grid, the device or the run -- and there are no floating-point atomics: the result is bitwise repeatable.
// W_T's LDS rows are k | 1 doubles long (odd: the 32 rows of a half-wave read 32 distinct bank pairs); H's tile is read at one
// address per half-wave (a broadcast).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rgraph {

constexpr int NT = 256;
constexpr int TILE = 32;
constexpr int GRAPH_MAX_BRANCHES = 8;
constexpr int GRAPH_MAX_K = 128;
constexpr int LOSS_ROWS = 32;          // rows of X per workgroup
constexpr int LOSS_CT = 16;            // columns of H staged at a time: NT / LOSS_ROWS column groups x 2 columns
enum { GRAPH_CONCAT = 0, GRAPH_ADD = 1 };

struct AssembleArgs {
    const double* H[GRAPH_MAX_BRANCHES];
    int kb[GRAPH_MAX_BRANCHES];
    int off[GRAPH_MAX_BRANCHES];       // concat: first output column of the branch
    int nb, mode;
    int kcols;                         // output columns before the condition block
    const double* Z;
    int p;
};

// grid: (tiles over n, tiles over c)
__global__ __launch_bounds__(NT) void graph_assemble_kernel(AssembleArgs a, int64_t n, double* __restrict__ X) {
    __shared__ double tile[TILE][TILE + 1];
    const int c_total = a.kcols + a.p;
    const int64_t j0 = (int64_t)blockIdx.x * TILE;
    const int c0 = blockIdx.y * TILE;
    const int tx = threadIdx.x % TILE, ty = threadIdx.x / TILE;
    // read: tx runs over the output columns (features), ty over the samples
    const int cc = c0 + tx;
    const double* src = nullptr;
    int ld = 0, f = 0;
    if (cc < c_total) {
        if (cc >= a.kcols) { src = a.Z; ld = a.p; f = cc - a.kcols; }
        else if (a.mode == GRAPH_ADD) { ld = a.kb[0]; f = cc; }
        else {
            int b = 0;
            while (b + 1 < a.nb && cc >= a.off[b + 1]) ++b;
            src = a.H[b]; ld = a.kb[b]; f = cc - a.off[b];
        }
    }
    for (int r = ty; r < TILE; r += NT / TILE) {
        const int64_t j = j0 + r;
        double v = 0.0;
        if (cc < c_total && j < n) {
            if (src) v = src[j * ld + f];
            else {
                v = a.H[0][j * ld + f];
                for (int b = 1; b < a.nb; ++b) v += a.H[b][j * ld + f];
            }
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    // write: tx runs over the samples, ty over the output columns
    const int64_t j = j0 + tx;
    for (int r = ty; r < TILE; r += NT / TILE) {
        const int co = c0 + r;
        if (co < c_total && j < n) X[(int64_t)co * n + j] = tile[tx][r];
    }
}

// fixed-order tree over the workgroup's NT values; the result is in sh[0]
__device__ __forceinline__ void block_tree_sum(double* sh) {
    for (int w = NT / 2; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    }
    __syncthreads();
}

__host__ __device__ inline int loss_ldw(int k) { return k | 1; }
inline size_t loss_lds_bytes(int k) { return ((size_t)LOSS_ROWS * loss_ldw(k) + (size_t)LOSS_CT * k + NT) * sizeof(double); }

// grid: ceil(rows / LOSS_ROWS) workgroups; partial: one double per workgroup.  Dynamic LDS: loss_lds_bytes(k).
__global__ __launch_bounds__(NT) void graph_layer_loss_kernel(const double* __restrict__ X, int64_t rows, int c,
                                                               const double* __restrict__ W_T, const double* __restrict__ d,
                                                               const double* __restrict__ H, int k, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* Ws = reinterpret_cast<double*>(smem_raw);                  // LOSS_ROWS x ldw: W_T[f, row] * d[f]
    const int ldw = loss_ldw(k);
    double* Hs = Ws + (size_t)LOSS_ROWS * ldw;                         // LOSS_CT x k
    double* red = Hs + (size_t)LOSS_CT * k;                            // NT
    const int64_t i0 = (int64_t)blockIdx.x * LOSS_ROWS;
    const int nrow = (int)(rows - i0 < LOSS_ROWS ? rows - i0 : LOSS_ROWS);
    for (int e = threadIdx.x; e < LOSS_ROWS * k; e += NT) {
        const int r = e / k, f = e - r * k;
        Ws[r * ldw + f] = r < nrow ? W_T[i0 * k + e] * d[f] : 0.0;
    }
    const int r = threadIdx.x % LOSS_ROWS, cg = threadIdx.x / LOSS_ROWS;
    const double* w = Ws + r * ldw;
    double sq = 0.0;
    for (int ct = 0; ct < c; ct += LOSS_CT) {
        const int ncol = c - ct < LOSS_CT ? c - ct : LOSS_CT;
        __syncthreads();                                               // the previous tile has been read (first pass: Ws is written)
        for (int e = threadIdx.x; e < ncol * k; e += NT) Hs[e] = H[(int64_t)ct * k + e];
        __syncthreads();
        const int ca = 2 * cg, cb = 2 * cg + 1;
        if (r < nrow && ca < ncol) {
            const double* ha = Hs + ca * k;
            const double* hb = Hs + (cb < ncol ? cb : ca) * k;
            double pa = 0.0, pb = 0.0;
            for (int f = 0; f < k; ++f) {
                const double wv = w[f];
                pa += wv * ha[f];
                pb += wv * hb[f];
            }
            const double da = X[(int64_t)(ct + ca) * rows + i0 + r] - pa;
            sq += da * da;
            if (cb < ncol) {
                const double db = X[(int64_t)(ct + cb) * rows + i0 + r] - pb;
                sq += db * db;
            }
        }
    }
    __syncthreads();
    red[threadIdx.x] = sq;
    block_tree_sum(red);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup: thread t adds its segment of ceil(count / NT) consecutive partials in index order, then the tree;
// out[0] = scale * sum
__global__ __launch_bounds__(NT) void graph_loss_final_kernel(const double* __restrict__ partial, int64_t count, double scale,
                                                               double* __restrict__ out) {
    __shared__ double sh[NT];
    const int64_t seg = (count + NT - 1) / NT;
    const int64_t q0 = (int64_t)threadIdx.x * seg;
    const int64_t q1 = q0 + seg < count ? q0 + seg : count;
    double s = 0.0;
    for (int64_t q = q0; q < q1; ++q) s += partial[q];
    sh[threadIdx.x] = s;
    block_tree_sum(sh);
    if (threadIdx.x == 0) out[0] = scale * sh[0];
}

// out[0] = scale * in[0]  and  total[0] = sum of v[0 .. count) in index order: the two scalar steps of the outer loop's loss
__global__ void graph_scale_scalar_kernel(const double* __restrict__ in, double scale, double* __restrict__ out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = scale * in[0];
}
__global__ void graph_sum_scalars_kernel(const double* __restrict__ v, int count, double* __restrict__ total) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < count; ++q) s += v[q];
        total[0] = s;
    }
}

}  // namespace rgraph
