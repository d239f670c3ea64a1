// kernels_refine.hip.h -- the label-dependent stages of compute_target() / refine() (ops_refine.hip), fp64.
//
// Centroid sums.  The host sorts the labelled columns by class (a stable counting sort: `perm`) and cuts every class into chunks of
// CHUNK columns; chunk q covers perm[chunk_start[q] .. chunk_start[q] + chunk_len[q]).  centroid_partial_kernel: one workgroup per
// chunk; thread (slot, f) adds feature f of the chunk's columns slot, slot + slots, ... in that order, then slot 0 adds the slots'
// sums in slot order.  centroid_final_kernel adds a class's chunk partials in chunk order.  No atomics, and the order of every
// addition is a function of (k, the class layout) alone: the sums do not depend on the grid, the device or the run.
//
// Correction.  add_table_kernel: out[f, j] = (H ? H[f, j] : 0) + table[f, label_j] (0 for an unlabelled column), clipped at 0 when
// asked; the k x C table sits in LDS when it fits.  One read of H, one write.
//
// sumsq_chunk_kernel / sum_chunks_kernel: ||H||_F^2 over fixed chunks of SQ_CHUNK elements, chunk partials added in chunk order.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rref {

constexpr int NT = 256;
constexpr int CHUNK = 256;            // columns of one class per workgroup
constexpr int SQ_CHUNK = 4096;        // elements per workgroup of the sum of squares
constexpr size_t TABLE_LDS_MAX = 48 * 1024;

// feature stride of the (slot, f) thread layout: the power of two >= k, at most NT
__host__ __device__ inline int feat_stride(int k) {
    int s = 1;
    while (s < k && s < NT) s <<= 1;
    return s;
}

// partial: nchunks x k.  LDS: NT doubles.
__global__ __launch_bounds__(NT) void centroid_partial_kernel(const double* __restrict__ H, int k, const int* __restrict__ perm,
                                                               const int* __restrict__ chunk_start,
                                                               const int* __restrict__ chunk_len, double* __restrict__ partial) {
    __shared__ double sh[NT];
    const int q = blockIdx.x;
    const int start = chunk_start[q], len = chunk_len[q];
    const int fs = feat_stride(k);
    const int slots = NT / fs;
    const int f0 = threadIdx.x % fs, slot = threadIdx.x / fs;
    for (int fb = 0; fb < k; fb += fs) {              // one pass unless k > NT
        const int f = fb + f0;
        double s = 0.0;
        if (f < k)
            for (int c = slot; c < len; c += slots) s += H[(int64_t)perm[start + c] * k + f];
        sh[threadIdx.x] = s;
        __syncthreads();
        if (slot == 0 && f < k) {
            double t = sh[f0];
            for (int u = 1; u < slots; ++u) t += sh[u * fs + f0];
            partial[(int64_t)q * k + f] = t;
        }
        __syncthreads();
    }
}

// sums: k x C.  class_chunk_ptr: C + 1 (the chunks of class c are class_chunk_ptr[c] .. class_chunk_ptr[c + 1]).
__global__ __launch_bounds__(NT) void centroid_final_kernel(const double* __restrict__ partial, int k, int C,
                                                             const int* __restrict__ class_chunk_ptr, double* __restrict__ sums) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= (int64_t)k * C) return;
    const int c = (int)(e / k), f = (int)(e % k);
    double s = 0.0;
    for (int q = class_chunk_ptr[c]; q < class_chunk_ptr[c + 1]; ++q) s += partial[(int64_t)q * k + f];
    sums[e] = s;
}

template <bool IN_LDS>
__global__ __launch_bounds__(NT) void add_table_kernel(const double* __restrict__ H, const int* __restrict__ labels,
                                                        const double* __restrict__ table, int k, int C, int64_t n, int nonneg,
                                                        double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const double* tab = table;
    if (IN_LDS) {
        double* sh = reinterpret_cast<double*>(smem_raw);
        for (int e = threadIdx.x; e < k * C; e += NT) sh[e] = table[e];
        __syncthreads();
        tab = sh;
    }
    const int64_t total = (int64_t)k * n;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t j = e / k;
        const int f = (int)(e - j * k);
        const int lab = labels[j];
        double v = H ? H[e] : 0.0;
        if (lab >= 0 && lab < C) v += tab[(int64_t)lab * k + f];
        if (nonneg && v < 0.0) v = 0.0;
        out[e] = v;
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

__global__ __launch_bounds__(NT) void sumsq_chunk_kernel(const double* __restrict__ x, int64_t len, double* __restrict__ partial) {
    __shared__ double sh[NT];
    const int64_t base = (int64_t)blockIdx.x * SQ_CHUNK;
    double s = 0.0;
    for (int u = 0; u < SQ_CHUNK / NT; ++u) {
        const int64_t e = base + (int64_t)u * NT + threadIdx.x;
        if (e < len) { const double v = x[e]; s += v * v; }
    }
    sh[threadIdx.x] = s;
    block_tree_sum(sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

// one workgroup: thread t adds partials t, t + NT, ... in that order, then the tree
__global__ __launch_bounds__(NT) void sum_chunks_kernel(const double* __restrict__ partial, int64_t count, double* __restrict__ out) {
    __shared__ double sh[NT];
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < count; q += NT) s += partial[q];
    sh[threadIdx.x] = s;
    block_tree_sum(sh);
    if (threadIdx.x == 0) out[0] = sh[0];
}

// d[f] = max(sqrt(ss[f]), floor)
__global__ void norm_floor_kernel(const double* __restrict__ ss, int k, double floor_v, double* __restrict__ d) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= k) return;
    const double v = sqrt(ss[f]);
    d[f] = v < floor_v ? floor_v : v;
}

// X[f, j] = X[f, j] / d[f] (DIV) or X[f, j] * d[f]
template <bool DIV>
__global__ __launch_bounds__(NT) void scale_rows_kernel(double* __restrict__ X, int k, int64_t total, const double* __restrict__ d) {
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const double dv = d[e % k];
        X[e] = DIV ? X[e] / dv : X[e] * dv;
    }
}

}  // namespace rref
