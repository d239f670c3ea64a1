// kernels_consensus.hip.h -- device side of consensus clustering (ops_consensus.hip): the consensus stage of the reference's
// consensus_nmf (R/consensus.R:102-129) and its c_knn_jaccard (src/RcppFunctions_utils.cpp:560-618).  W_r is the loading of
// replicate r, m samples x k factors, stored k-major (sample i: k contiguous values), the stack replicate after replicate.
//
//   labels_kernel       hard: label[r][i] = first maximum of row i of W_r (R's which.max: ties to the lowest index)
//   hard_tile_kernel    hard: a 64 x 64 tile of consensus; the two label strips of 16 replicates at a time staged in LDS, an integer
//                       count per (i, j) over all replicates, one fp64 division on store; every element written exactly once
//   normalize_kernel    knn_jaccard: rows scaled to unit 2-norm (fp64, squares added in factor order, W / sqrt(sum))
//   sim_tile_kernel     knn_jaccard: a 64 x 64 tile of sim = Wn Wn^T for a strip of rows (an FMA chain over the factors in order
//                       from LDS panels), into the strip scratch
//   select_kernel       knn_jaccard: one wavefront per row: the actual_k-th largest similarity by bisection on the 64 bits of the
//                       order-preserving key (exact for every actual_k), then the neighbour set as a bitset of ceil(m / 64) words
//   jaccard_tile_kernel knn_jaccard: a 64 x 64 tile of J from AND + popcount over the two bitset strips (staged in LDS 16 words at a
//                       time), added into the fp64 accumulator; the last replicate stores (acc + J) / reps
//
// The two rules of this build where the reference is undefined: equal similarities go to the lower index (std::partial_sort leaves
// ties unspecified), and a row of W_r with zero norm has similarity 0 to every sample (R's 0 / 0 gives NaN rows).
//
// No atomics.  Every floating-point value has one fixed order of operations (the similarity of (i, j) is the same chain as that of
// (j, i), so sim, J and the consensus are bitwise symmetric); J is added in replicate order.  Indices into m x m arrays are 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rcons {

constexpr int T = 64;        // tile edge
constexpr int NT = 256;      // threads per tile workgroup: 16 x 16, 4 x 4 entries each
constexpr int KC = 16;       // factors per LDS panel
constexpr int RC = 16;       // replicates per LDS stage (hard)
constexpr int WC = 16;       // bitset words per LDS stage (knn_jaccard)

__global__ __launch_bounds__(NT) void labels_kernel(const double* __restrict__ W, int64_t rows, int k, int* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;      // row of the whole stack: r * m + i
    if (i >= rows) return;
    const double* w = W + i * k;
    double best = w[0];
    int arg = 0;
    for (int f = 1; f < k; ++f) {
        const double v = w[f];
        if (v > best) { best = v; arg = f; }
    }
    label[i] = arg;
}

__global__ __launch_bounds__(NT) void hard_tile_kernel(const int* __restrict__ label, int64_t m, int reps, double* __restrict__ out) {
    __shared__ int sI[RC][T];
    __shared__ int sJ[RC][T];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * T, r0 = (int64_t)blockIdx.y * T;    // columns j (fast in memory), rows i
    int cnt[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) cnt[a][b] = 0;
    for (int q0 = 0; q0 < reps; q0 += RC) {
#pragma unroll
        for (int q = 0; q < (RC * T) / NT; ++q) {
            const int idx = t + NT * q, e = idx % T, r = idx / T;
            const bool live = q0 + r < reps;
            // a replicate past the end never matches: -1 on one side, -2 on the other
            sI[r][e] = (live && r0 + e < m) ? label[(int64_t)(q0 + r) * m + r0 + e] : -1;
            sJ[r][e] = (live && c0 + e < m) ? label[(int64_t)(q0 + r) * m + c0 + e] : -2;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            int li[4], lj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { li[a] = sI[r][ty + 16 * a]; lj[a] = sJ[r][tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) cnt[a][b] += li[a] == lj[b] ? 1 : 0;
        }
        __syncthreads();
    }
    const double dr = (double)reps;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t gi = r0 + ty + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t gj = c0 + tx + 16 * b;
            if (gi < m && gj < m) out[gi * m + gj] = (double)cnt[a][b] / dr;
        }
    }
}

// in place over the whole stack (rows = reps * m)
__global__ __launch_bounds__(NT) void normalize_kernel(double* __restrict__ W, int64_t rows, int k) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= rows) return;
    double* w = W + i * k;
    double s = 0.0;
    for (int f = 0; f < k; ++f) s += w[f] * w[f];
    const double nrm = sqrt(s);
    for (int f = 0; f < k; ++f) w[f] = nrm > 0.0 ? w[f] / nrm : 0.0;
}

// sim rows [i0, i0 + nrows) x all m columns -> S (nrows x m, row-major).  grid: (column tiles, row tiles of the strip)
__global__ __launch_bounds__(NT) void sim_tile_kernel(const double* __restrict__ Wn, int64_t m, int k, int64_t i0, int64_t nrows,
                                                      double* __restrict__ S) {
    __shared__ double sA[KC][T + 1];
    __shared__ double sB[KC][T + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * T, r0 = i0 + (int64_t)blockIdx.y * T;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int f0 = 0; f0 < k; f0 += KC) {
#pragma unroll
        for (int q = 0; q < (KC * T) / NT; ++q) {
            const int idx = t + NT * q, r = idx / KC, f = idx % KC;
            const int64_t gi = r0 + r, gj = c0 + r;
            sA[f][r] = (gi < i0 + nrows && f0 + f < k) ? Wn[gi * k + f0 + f] : 0.0;
            sB[f][r] = (gj < m && f0 + f < k) ? Wn[gj * k + f0 + f] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < KC; ++f) {
            double av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { av[a] = sA[f][ty + 16 * a]; bv[a] = sB[f][tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t gi = r0 + ty + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t gj = c0 + tx + 16 * b;
            if (gi < i0 + nrows && gj < m) S[(gi - i0) * m + gj] = acc[a][b] + 0.0;      // an underflowed -0 becomes +0
        }
    }
}

// order-preserving key of a finite double: a > b  <=>  key(a) > key(b)  (-0 does not occur: sim_tile_kernel stores v + 0)
__device__ __forceinline__ unsigned long long sim_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wavefront per row of the strip.  The neighbour set of row i: the K largest sim[i][j], j != i, equal values to the lower j.
// thr = the K-th largest key = the largest t with #{j != i : key_j >= t} >= K, found a bit at a time from the top; then every j
// above thr, and the first K - #{above} of those equal to it in index order.  bits: nrows x words.
__global__ __launch_bounds__(NT) void select_kernel(const double* __restrict__ S, int64_t m, int64_t i0, int64_t nrows, int K,
                                                    int64_t words, unsigned long long* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= nrows) return;                                  // whole wavefronts leave together
    const int64_t self = i0 + row;
    const double* s = S + row * m;
    unsigned long long thr = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = thr | (1ull << bit);
        int c = 0;
        for (int64_t j = lane; j < m; j += 64) c += (j != self && sim_key(s[j]) >= cand) ? 1 : 0;
        if (wave_sum(c) >= K) thr = cand;
    }
    int above = 0;
    for (int64_t j = lane; j < m; j += 64) above += (j != self && sim_key(s[j]) > thr) ? 1 : 0;
    int need = K - wave_sum(above);                            // >= 1 of the values equal to thr
    unsigned long long* out = bits + (self)*words;
    for (int64_t w = 0; w < words; ++w) {
        const int64_t j = w * 64 + lane;
        const bool live = j < m && j != self;
        const unsigned long long key = live ? sim_key(s[j]) : 0ull;
        const unsigned long long eq = __ballot(live && key == thr);
        const int before = __popcll(eq & ((1ull << lane) - 1ull));
        const bool in = live && (key > thr || (key == thr && before < need));
        const unsigned long long word = __ballot(in);
        need -= min(need, (int)__popcll(eq));
        if (lane == 0) out[w] = word;
    }
}

// acc (m x m) += J of this replicate; first: acc is not read (it starts from 0 + J = J); last: (acc + J) / reps is stored
__global__ __launch_bounds__(NT) void jaccard_tile_kernel(const unsigned long long* __restrict__ bits, int64_t m, int64_t words, int K,
                                                          int first, int last, double reps, double* __restrict__ acc) {
    __shared__ unsigned long long sI[WC][T + 1];
    __shared__ unsigned long long sJ[WC][T + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int64_t c0 = (int64_t)blockIdx.x * T, r0 = (int64_t)blockIdx.y * T;
    int inter[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) inter[a][b] = 0;
    for (int64_t w0 = 0; w0 < words; w0 += WC) {
#pragma unroll
        for (int q = 0; q < (WC * T) / NT; ++q) {
            const int idx = t + NT * q, w = idx % WC, e = idx / WC;
            const bool live = w0 + w < words;
            sI[w][e] = (live && r0 + e < m) ? bits[(r0 + e) * words + w0 + w] : 0ull;
            sJ[w][e] = (live && c0 + e < m) ? bits[(c0 + e) * words + w0 + w] : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WC; ++w) {
            unsigned long long bi[4], bj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { bi[a] = sI[w][ty + 16 * a]; bj[a] = sJ[w][tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) inter[a][b] += (int)__popcll(bi[a] & bj[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int64_t gi = r0 + ty + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t gj = c0 + tx + 16 * b;
            if (gi < m && gj < m) {
                const int un = 2 * K - inter[a][b];
                const double J = gi == gj ? 1.0 : (un > 0 ? (double)inter[a][b] / (double)un : 0.0);
                const double v = (first ? 0.0 : acc[gi * m + gj]) + J;
                acc[gi * m + gj] = last ? v / reps : v;
            }
        }
    }
}

}  // namespace rcons
