// kernels_classify_rf.hip.h -- device kernels of the histogram random forest (ops_classify_rf.hip).  Every count is
// an integer; the only floating-point steps are the binning and the split score, each one fp64 expression without a multiply-add to
// contract.  Integer LDS / global adds are order-free, every choice is taken by a fixed rule, so the forest is bitwise repeatable and
// independent of the grid, of the tree batch and of the small / large switch.
//
//   rf_minmax / rf_bin        per-feature minimum and maximum of the training rows; bins as uint8, feature-major (p x rows).
//   rf_bootstrap / rf_root    multiplicities per (tree, row) by integer atomics from the counter-based SplitMix64 draws; the in-bag
//                             rows of a tree, compacted in row order, are the root's segment of (row, multiplicity) entries.
//   rf_search<WPI, CNT>       one level's split search: a work item is one active (tree, node).  Class totals first (purity, the
//                             majority class), then the node's mtry candidate features one after the other: the C x 256 class-by-bin
//                             histogram of multiplicities is built in LDS by integer adds, each lane owns four bins, one wave prefix
//                             sum per class gives L_c(t), accumulated as int64 S_L, S_R and N_L per threshold, the fp64 score is
//                             formed and a wave argmax keeps (score, t) under the tie rule.  WPI = 4, CNT = uint32: one workgroup
//                             per node, its four waves share the segment and split the classes (long segments).  WPI = 1,
//                             CNT = uint16: one wave per node, four nodes per workgroup (at most SMALL_MAX entries and SMALL_BAG
//                             in-bag rows).  Which of the two runs a node changes no result.
//   rf_tree_scan / rf_offsets child ids by a prefix sum over a tree's split nodes of the level, then the trees' offsets into the next
//                             level's work list, which therefore stays in (tree, node) order.
//   rf_partition              one wave per split node: a stable left / right split of its segment into the other entry buffer by
//                             ballots and prefix counts; writes the node record, the children's segments and work items.
//   rf_predict                one thread per (test row, tree); the tree's node records pass through LDS when they fit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rrf {

constexpr int THREADS = 256;
constexpr int NBIN = 256;
constexpr int MAX_DEPTH = 40;
constexpr int SMALL_MAX = 128;         // entries of a segment the one-wave search takes
constexpr int SMALL_BAG = 65535;       // ... and its in-bag count (uint16 counters)
constexpr int LDS_NODES = 4096;        // node records rf_predict stages in LDS (64 KiB)
constexpr int CMAX = 64, PMAX = 128;

__host__ __device__ inline bool is_large(int cnt, int nbag) { return cnt > SMALL_MAX || nbag > SMALL_BAG; }

// draw q of the SplitMix64 stream (rng/rng.hpp:89-104): uniform<double>() = double(next()) / 2^64
__device__ inline double draw(uint64_t seed, uint64_t q) {
    uint64_t z = seed + (q + 1) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z = z ^ (z >> 31);
    return (double)z / 18446744073709551616.0;
}

__device__ inline int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive prefix of v over the THREADS threads of the block, their sum in `total`.  sh: 4 ints of LDS.
__device__ inline int block_excl_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += sh[i];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return off + inc - v;
}

// ---------------------------------------------------------------------------------------------------------------- binning
// Grid = p.  X: n x p row-major.  Minimum and maximum are exact whatever the order.
__global__ __launch_bounds__(THREADS) void rf_minmax(const double* __restrict__ X, int n, int p, double* __restrict__ lo,
                                                     double* __restrict__ hi) {
    __shared__ double smn[THREADS], smx[THREADS];
    const int f = blockIdx.x, tid = threadIdx.x;
    double mn = X[f], mx = X[f];
    for (int r = tid; r < n; r += THREADS) {
        const double v = X[(size_t)r * p + f];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    smn[tid] = mn; smx[tid] = mx;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            smn[tid] = smn[tid + s] < smn[tid] ? smn[tid + s] : smn[tid];
            smx[tid] = smx[tid + s] > smx[tid] ? smx[tid + s] : smx[tid];
        }
        __syncthreads();
    }
    if (tid == 0) { lo[f] = smn[0]; hi[f] = smx[0]; }
}

// out[f * n + row]: v = (x - lo) * (256 / (hi - lo)); 255 when v >= 255, floor(v) when v > 0, else 0 (NaN included); 0 when hi == lo
__global__ __launch_bounds__(THREADS) void rf_bin(const double* __restrict__ X, int n, int p, const double* __restrict__ lo,
                                                  const double* __restrict__ hi, uint8_t* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (size_t)n * p) return;
    const int f = (int)(e / n), row = (int)(e % n);
    const double l = lo[f], h = hi[f];
    int b = 0;
    if (h != l) {
        const double scale = 256.0 / (h - l);
        const double v = (X[(size_t)row * p + f] - l) * scale;
        b = v >= 255.0 ? 255 : (v > 0.0 ? (int)v : 0);
    }
    out[e] = (uint8_t)b;
}

// ---------------------------------------------------------------------------------------------------------------- bootstrap
// Grid (ceil(n / THREADS), B).  mult (B x n, zeroed): tree t0 + blockIdx.y takes draws (t0 + blockIdx.y) n + i.
__global__ __launch_bounds__(THREADS) void rf_bootstrap(uint64_t seed, int t0, int n, uint32_t* __restrict__ mult) {
    const int i = blockIdx.x * THREADS + threadIdx.x, tb = blockIdx.y;
    if (i >= n) return;
    const double u = draw(seed, (uint64_t)(t0 + tb) * (uint64_t)n + (uint64_t)i);
    long long row = (long long)(u * (double)n);
    if (row > n - 1) row = n - 1;
    atomicAdd(&mult[(size_t)tb * n + row], 1u);
}

struct GrowArgs {
    const uint8_t* bins;          // p x n
    const uint8_t* y;             // n class codes
    const uint2* ent;             // B x n (row, multiplicity) entries of this level, grouped by node
    uint2* ent_next;              // ... of the next
    int4* seg;                    // B x 2n: (start, entries, in-bag count, -)
    int4* nodes;                  // B x 2n: (feature, threshold, left child, majority class); a leaf: (-1, -1, -1, class)
    int4* rec;                    // per work item: (feature or -1, threshold, N_L, majority class)
    int* child;                   // per work item: the left child's id, -1 for a leaf
    const int2* act;              // work items (tree of the batch, node) in (tree, node) order
    int2* act_next;
    const int* act_off;           // B + 1: a tree's range of work items
    int* act_off_next;
    const int* large;             // work items the workgroup search takes, in any order
    int* large_next;
    int* counters;                // [0] work items, [1] large ones of the next level
    int* ncount;                  // B: nodes of a tree
    int* lvl_base;                // B: ncount before this level's children
    int* nsplit;                  // B: split nodes of this level
    int n, p, C, mtry, B, t0, ntree, level, n_active, n_large;
    uint64_t seed;
};

// Grid = B.  The in-bag rows of a tree in row order; node 0; work item tb.  counters[1] is zero on entry.
__global__ __launch_bounds__(THREADS) void rf_root(const uint32_t* __restrict__ mult, GrowArgs a) {
    __shared__ int sh[4];
    const int tb = blockIdx.x, tid = threadIdx.x, n = a.n;
    uint2* ent = a.ent_next + (size_t)tb * n;
    int base = 0;
    for (int r0 = 0; r0 < n; r0 += THREADS) {
        const int row = r0 + tid;
        const uint32_t w = row < n ? mult[(size_t)tb * n + row] : 0u;
        int tot;
        const int ex = block_excl_scan(w > 0, sh, tot);
        if (w > 0) ent[base + ex] = make_uint2((uint32_t)row, w);
        base += tot;
    }
    if (tid == 0) {
        a.seg[(size_t)tb * 2 * n] = make_int4(0, base, n, 0);
        a.ncount[tb] = 1;
        a.act_next[tb] = make_int2(tb, 0);
        a.act_off_next[tb] = tb;
        if (tb == 0) { a.act_off_next[a.B] = a.B; a.counters[0] = a.B; }
        if (is_large(base, n)) a.large_next[atomicAdd(&a.counters[1], 1)] = tb;
    }
}

// ---------------------------------------------------------------------------------------------------------------- split search
template <int WPI> __device__ inline void item_sync() {
    if constexpr (WPI == 4) {
        __syncthreads();
    } else {                                 // one wave owns the item: its LDS operations complete in order
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// bytes of dynamic LDS: per item the histogram, 64 class totals and 128 candidate features; WPI = 4 adds the S_L, S_R, N_L sums
__host__ __device__ inline size_t rf_item_bytes(int C, size_t cnt_bytes) { return (size_t)C * NBIN * cnt_bytes + CMAX * 4 + PMAX; }
__host__ __device__ inline size_t rf_search_lds(int C, int wpi) {
    return wpi == 4 ? rf_item_bytes(C, 4) + (size_t)NBIN * 20 : 4 * rf_item_bytes(C, 2);
}

template <int WPI, class CNT>
__global__ __launch_bounds__(THREADS) void rf_search(GrowArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = WPI * 64;                       // threads of an item
    constexpr int IPW = THREADS / NT;                  // items of a workgroup
    const int tid = threadIdx.x, sub = tid / NT, it = tid % NT, lane = tid & 63, wv = it >> 6;
    const int C = a.C, n = a.n, p = a.p;
    const size_t hist_bytes = (size_t)C * NBIN * sizeof(CNT), item_bytes = rf_item_bytes(C, sizeof(CNT));
    unsigned char* base = smem + (size_t)sub * item_bytes;
    uint32_t* histw = reinterpret_cast<uint32_t*>(base);
    uint32_t* tot = reinterpret_cast<uint32_t*>(base + hist_bytes);
    uint8_t* cand = reinterpret_cast<uint8_t*>(tot + CMAX);
    unsigned long long* SLr = reinterpret_cast<unsigned long long*>(smem + (size_t)IPW * item_bytes);      // WPI = 4 only
    unsigned long long* SRr = SLr + NBIN;
    uint32_t* NLr = reinterpret_cast<uint32_t*>(SRr + NBIN);

    int ai;
    if constexpr (WPI == 4) {
        ai = a.large[blockIdx.x];
    } else {
        ai = blockIdx.x * IPW + sub;
        if (ai >= a.n_active) return;                  // whole waves leave: no block barrier below
    }
    const int2 who = a.act[ai];
    const int tb = who.x, node = who.y;
    const int4 sg = a.seg[(size_t)tb * 2 * n + node];
    const int cnt = sg.y, nbag = sg.z;
    if constexpr (WPI == 1) {
        if (is_large(cnt, nbag)) return;
    }
    const uint2* e = a.ent + (size_t)tb * n + sg.x;

    // class totals, purity, majority class (first maximum)
    for (int c = it; c < CMAX; c += NT) tot[c] = 0;
    item_sync<WPI>();
    for (int i = it; i < cnt; i += NT) {
        const uint2 en = e[i];
        atomicAdd(&tot[a.y[en.x]], en.y);
    }
    item_sync<WPI>();
    int cls = 0, nz = 0;
    uint32_t bestc = 0;
    for (int c = 0; c < C; ++c) {
        const uint32_t v = tot[c];
        nz += v > 0;
        if (v > bestc) { bestc = v; cls = c; }
    }
    double bs = -1.0;
    int bf = -1, bt = -1, bnl = 0;
    if (nz > 1 && nbag >= 2 && a.level < MAX_DEPTH) {
        // candidate features: partial Fisher-Yates over 0 .. p - 1
        for (int j = it; j < p; j += NT) cand[j] = (uint8_t)j;
        item_sync<WPI>();
        if (it == 0) {
            const uint64_t q0 = (uint64_t)a.ntree * (uint64_t)n + ((uint64_t)(a.t0 + tb) * 2ull * (uint64_t)n + (uint64_t)node) * (uint64_t)p;
            for (int i = 0; i < a.mtry; ++i) {
                const double u = draw(a.seed, q0 + i);
                int j = i + (int)(u * (double)(p - i));
                if (j > p - 1) j = p - 1;
                const uint8_t x = cand[i]; cand[i] = cand[j]; cand[j] = x;
            }
        }
        item_sync<WPI>();
        const int nwords = (int)(hist_bytes / 4);
        for (int ci = 0; ci < a.mtry; ++ci) {
            const int f = cand[ci];
            for (int i = it; i < nwords; i += NT) histw[i] = 0;
            if constexpr (WPI == 4) { SLr[it] = 0; SRr[it] = 0; NLr[it] = 0; }
            item_sync<WPI>();
            const uint8_t* bf8 = a.bins + (size_t)f * n;
            for (int i = it; i < cnt; i += NT) {
                const uint2 en = e[i];
                const int b = bf8[en.x], c = a.y[en.x];
                if constexpr (sizeof(CNT) == 4) atomicAdd(&histw[c * NBIN + b], en.y);
                else atomicAdd(&histw[c * (NBIN / 2) + (b >> 1)], en.y << ((b & 1) * 16));      // a half never carries: nbag <= 65535
            }
            item_sync<WPI>();
            // lane owns thresholds 4 lane .. 4 lane + 3; wave wv of the item takes classes wv, wv + WPI, ...
            long long SL[4] = {0, 0, 0, 0}, SR[4] = {0, 0, 0, 0};
            uint32_t NL[4] = {0, 0, 0, 0};
            for (int c = wv; c < C; c += WPI) {
                const uint32_t tc = tot[c];
                if (tc == 0) continue;                 // wave-uniform
                uint32_t h[4];
                if constexpr (sizeof(CNT) == 4) {
                    const uint4 v = *reinterpret_cast<const uint4*>(histw + c * NBIN + 4 * lane);
                    h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
                } else {
                    const uint2 v = *reinterpret_cast<const uint2*>(histw + c * (NBIN / 2) + 2 * lane);
                    h[0] = v.x & 0xffffu; h[1] = v.x >> 16; h[2] = v.y & 0xffffu; h[3] = v.y >> 16;
                }
                h[1] += h[0]; h[2] += h[1]; h[3] += h[2];
                const uint32_t ex = (uint32_t)wave_incl_scan((int)h[3]) - h[3];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long L = (long long)(ex + h[k]), R = (long long)tc - L;
                    SL[k] += L * L; SR[k] += R * R; NL[k] += (uint32_t)L;
                }
            }
            if constexpr (WPI == 4) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    atomicAdd(&SLr[4 * lane + k], (unsigned long long)SL[k]);
                    atomicAdd(&SRr[4 * lane + k], (unsigned long long)SR[k]);
                    atomicAdd(&NLr[4 * lane + k], NL[k]);
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < 4; ++k) { SL[k] = (long long)SLr[4 * lane + k]; SR[k] = (long long)SRr[4 * lane + k]; NL[k] = NLr[4 * lane + k]; }
            }
            if (wv == 0) {
                double s = -1.0;
                int t = 1 << 30, nl = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int tk = 4 * lane + k;
                    if (tk <= NBIN - 2 && NL[k] > 0 && NL[k] < (uint32_t)nbag) {
                        const double sc = (double)SL[k] / (double)NL[k] + (double)SR[k] / (double)((uint32_t)nbag - NL[k]);
                        if (sc > s) { s = sc; t = tk; nl = (int)NL[k]; }
                    }
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {     // wave argmax: larger score, then smaller t
                    const double os = __shfl_xor(s, d);
                    const int ot = __shfl_xor(t, d), onl = __shfl_xor(nl, d);
                    if (os > s || (os == s && ot < t)) { s = os; t = ot; nl = onl; }
                }
                if (s > bs || (s == bs && s > 0.0 && f < bf)) { bs = s; bf = f; bt = t; bnl = nl; }
            }
            item_sync<WPI>();                          // the histogram is cleared next
        }
    }
    if (it == 0) {
        a.rec[ai] = make_int4(bf, bt, bnl, cls);
        if (bf < 0) a.nodes[(size_t)tb * 2 * n + node] = make_int4(-1, -1, -1, cls);
    }
}

// ---------------------------------------------------------------------------------------------------------------- child ids
// Grid = B.  The split nodes of tree tb, in work-list (= node) order, take ids ncount, ncount + 2, ...
__global__ __launch_bounds__(THREADS) void rf_tree_scan(GrowArgs a) {
    __shared__ int sh[4];
    const int tb = blockIdx.x, tid = threadIdx.x;
    const int a0 = a.act_off[tb], a1 = a.act_off[tb + 1], base = a.ncount[tb];
    __syncthreads();
    int run = 0;
    for (int i0 = a0; i0 < a1; i0 += THREADS) {
        const int i = i0 + tid;
        const int f = i < a1 && a.rec[i].x >= 0;
        int tot;
        const int ex = block_excl_scan(f, sh, tot);
        if (i < a1) a.child[i] = f ? base + 2 * (run + ex) : -1;
        run += tot;
    }
    if (tid == 0) { a.lvl_base[tb] = base; a.nsplit[tb] = run; a.ncount[tb] = base + 2 * run; }
}

// One workgroup: the trees' offsets into the next work list (two items per split node) and its length.
__global__ __launch_bounds__(THREADS) void rf_offsets(GrowArgs a) {
    __shared__ int sh[4];
    const int tid = threadIdx.x;
    int run = 0;
    for (int t0 = 0; t0 < a.B; t0 += THREADS) {
        const int t = t0 + tid;
        const int v = t < a.B ? 2 * a.nsplit[t] : 0;
        int tot;
        const int ex = block_excl_scan(v, sh, tot);
        if (t < a.B) a.act_off_next[t] = run + ex;
        run += tot;
    }
    if (tid == 0) { a.act_off_next[a.B] = run; a.counters[0] = run; a.counters[1] = 0; }
}

// ---------------------------------------------------------------------------------------------------------------- partition
// One wave per work item, four per workgroup.  A split node's entries go, in order, left (bin <= threshold) then right.
__global__ __launch_bounds__(THREADS) void rf_partition(GrowArgs a) {
    const int lane = threadIdx.x & 63, ai = blockIdx.x * 4 + (threadIdx.x >> 6), n = a.n;
    if (ai >= a.n_active) return;
    const int4 r = a.rec[ai];
    if (r.x < 0) return;
    const int2 who = a.act[ai];
    const int tb = who.x, node = who.y, left = a.child[ai];
    const int4 sg = a.seg[(size_t)tb * 2 * n + node];
    const int start = sg.x, cnt = sg.y;
    const uint2* e = a.ent + (size_t)tb * n + start;
    uint2* out = a.ent_next + (size_t)tb * n + start;
    const uint8_t* bf8 = a.bins + (size_t)r.x * n;
    int nle = 0;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        const bool go = i < cnt && bf8[e[i].x] <= r.y;
        nle += __popcll(__ballot(go));
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int pl = 0, pr = 0;
    for (int i0 = 0; i0 < cnt; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < cnt;
        uint2 en = make_uint2(0u, 0u);
        bool go = false;
        if (valid) { en = e[i]; go = bf8[en.x] <= r.y; }
        const unsigned long long ml = __ballot(valid && go), mr = __ballot(valid && !go);
        if (valid) out[go ? pl + __popcll(ml & below) : nle + pr + __popcll(mr & below)] = en;
        pl += __popcll(ml); pr += __popcll(mr);
    }
    if (lane == 0) {
        int4* seg = a.seg + (size_t)tb * 2 * n;
        a.nodes[(size_t)tb * 2 * n + node] = make_int4(r.x, r.y, left, r.w);
        seg[left] = make_int4(start, nle, r.z, 0);
        seg[left + 1] = make_int4(start + nle, cnt - nle, sg.z - r.z, 0);
        const int pos = a.act_off_next[tb] + (left - a.lvl_base[tb]);
        a.act_next[pos] = make_int2(tb, left);
        a.act_next[pos + 1] = make_int2(tb, left + 1);
        if (is_large(nle, r.z)) a.large_next[atomicAdd(&a.counters[1], 1)] = pos;
        if (is_large(cnt - nle, sg.z - r.z)) a.large_next[atomicAdd(&a.counters[1], 1)] = pos + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- prediction
// Grid (ceil(n_test / THREADS), B), LDS_NODES records of dynamic LDS.  tbins: p x n_test.  votes (n_test x C): integer atomics.
__global__ __launch_bounds__(THREADS) void rf_predict(const int4* __restrict__ nodes, const int* __restrict__ ncount, int n,
                                                      const uint8_t* __restrict__ tbins, int n_test, int C, int* __restrict__ votes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int4* sn = reinterpret_cast<int4*>(smem);
    const int tb = blockIdx.y, tid = threadIdx.x, row = blockIdx.x * THREADS + tid;
    const int4* nd = nodes + (size_t)tb * 2 * n;
    const int nc = ncount[tb];
    const bool staged = nc <= LDS_NODES;
    if (staged) {
        for (int i = tid; i < nc; i += THREADS) sn[i] = nd[i];
        __syncthreads();
    }
    if (row >= n_test) return;
    int node = 0;
    int4 r = staged ? sn[0] : nd[0];
    for (int d = 0; d < MAX_DEPTH && r.x >= 0; ++d) {          // a leaf is reached by depth 40
        node = r.z + (tbins[(size_t)r.x * n_test + row] <= r.y ? 0 : 1);
        r = staged ? sn[node] : nd[node];
    }
    atomicAdd(&votes[(size_t)row * C + r.w], 1);
}

}  // namespace rrf
