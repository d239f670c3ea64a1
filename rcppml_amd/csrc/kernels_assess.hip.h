// kernels_assess.hip.h -- device kernels of the embedding assessment entries (ops_assess.hip).  All fp32 with fp64 partial sums for
// k-means, no atomics: two runs are bitwise equal.
//
//   knn_partial / knn_merge   exact brute-force top-k.  A one-wave workgroup owns QPW queries and one contiguous candidate range
//                             (a split); each lane holds one candidate of a 64-candidate tile in VGPRs, the queries sit in LDS and
//                             are read by broadcast.  A query's running k-th distance lives in the VGPR of lane q, so most
//                             (query, candidate) pairs cost the distance and one compare; the survivors of a tile (a ballot) are
//                             inserted one by one, in candidate order, by the whole wave into the query's sorted list (LDS, or the
//                             partial output for lists that do not fit).  knn_merge merges the per-split lists by (d, index).
//   km_assign / km_accum / km_finalize   batched k-means (every restart in every launch): nearest centroid, per-block fp64 column
//                             sums in point order, block-ordered second stage and fp32 divide.
//   sil_kernel                one lane per point against the class samples, staged through LDS, summed per class in sample order.
//
// Distances are explicit __builtin_fmaf chains over j = 0 .. dim - 1 with diff = a - b, so -ffp-contract cannot change them.  Coordinates
// beyond dim are zero on both sides in the register paths: fmaf(0, 0, d) == d, so the padded chain is the unpadded one bit for bit.
// The fp32 sqrt and divisions are correctly rounded: hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt expands `/` and
// __builtin_sqrtf exactly (HIP's __fsqrt_rn is the approximate native sqrt unless OCML_BASIC_ROUNDED_OPERATIONS is defined).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ras {

constexpr int WAVE = 64;
constexpr float kBig = 1e30f;            // empty slot / initial threshold of the reference (never inserted: d >= kBig)

__device__ inline float rdlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ inline int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// ---------------------------------------------------------------------------------------------------------------- exact top-k
struct KnnArgs {
    const float* Q; const float* C;   // queries nq x dim, candidates nc x dim, row-major
    int nq, nc, dim;
    int mode;                         // 0 none, 1 exclude the query's own index, 2 exclude candidates of the query's group
    const int* group;                 // mode 2: group of every point (queries == candidates)
    const int* gk;                    // mode 2, may be null: k of a query = gk[group]
    int k, kmax;                      // k of every query without gk; list capacity (>= every query's k)
    int split_len;                    // candidates per split (multiple of 64)
    int qpw;                          // queries per workgroup (<= 64)
    int lists_lds;                    // 1: the lists live in LDS, 0: in the partial output
    float* pd; int* pi;               // partial lists [split][nq][kmax]
};

// k of query qi (0 .. kmax)
__device__ inline int knn_k(const KnnArgs& a, int qi) { return (a.mode == 2 && a.gk) ? a.gk[a.group[qi]] : a.k; }

// Insert (db, ib) into the sorted list L/I of length kq, below the current threshold.  Existing entries all have smaller candidate
// indices (candidates arrive in ascending order within a split), so ties go after them: position = #entries with d <= db.
__device__ inline void knn_insert(float* L, int* I, int kq, float db, int ib) {
    const int lane = threadIdx.x;
    int pos = 0;
    for (int s0 = 0; s0 < kq; s0 += WAVE) {
        const int s = s0 + lane;
        pos += __popcll(__ballot(s < kq && L[s] <= db));
    }
    for (int s0 = ((kq - 1) / WAVE) * WAVE; s0 >= 0; s0 -= WAVE) {   // top slots first: a round reads only slots not yet moved
        const int s = s0 + lane;
        const bool mv = s > pos && s < kq;
        float vd = 0.f; int vi = 0;
        if (mv) { vd = L[s - 1]; vi = I[s - 1]; }
        __syncthreads();
        if (mv) { L[s] = vd; I[s] = vi; }
        __syncthreads();
    }
    if (lane == 0) { L[pos] = db; I[pos] = ib; }
    __syncthreads();
}

// DB > 0: dim <= DB, candidate coordinates in VGPRs, queries in LDS (stride DB, zero padded).  DB == 0: any dim, both read from
// global memory.  Block = one wave.  Grid (ceil(nq / qpw), splits).
template <int DB> __global__ __launch_bounds__(WAVE) void knn_partial(KnnArgs a) {
    extern __shared__ float sm[];
    const int lane = threadIdx.x;
    const int q0 = blockIdx.x * a.qpw;
    const int nqb = min(a.qpw, a.nq - q0);
    const int c0 = blockIdx.y * a.split_len;
    const int c1 = min(a.nc, c0 + a.split_len);
    const size_t qsz = DB > 0 ? (size_t)a.qpw * DB : 0;
    const size_t obase = ((size_t)blockIdx.y * a.nq + q0) * a.kmax;
    float* qs = sm;
    float* Ld; int* Li;
    if (a.lists_lds) { Ld = sm + qsz; Li = reinterpret_cast<int*>(Ld + (size_t)a.qpw * a.kmax); }
    else { Ld = a.pd + obase; Li = a.pi + obase; }
    if (DB > 0)
        for (int e = lane; e < a.qpw * DB; e += WAVE) {
            const int q = e / DB, j = e % DB;
            qs[e] = (q < nqb && j < a.dim) ? a.Q[(size_t)(q0 + q) * a.dim + j] : 0.f;
        }
    for (int e = lane; e < nqb * a.kmax; e += WAVE) { Ld[e] = kBig; Li[e] = -1; }
    // lane q: query q's k, group and running threshold (k = 0: nothing is ever inserted)
    int myk = 0, mygrp = -1;
    float thr = -1.f;
    if (lane < nqb) {
        const int qi = q0 + lane;
        mygrp = a.mode == 2 ? a.group[qi] : -1;
        myk = knn_k(a, qi);
        thr = myk > 0 ? kBig : -1.f;
    }
    __syncthreads();
    for (int base = c0; base < c1; base += WAVE) {
        const int cand = base + lane;
        const bool cv = cand < c1;
        float c[DB > 0 ? DB : 1];
        if (DB > 0) {
#pragma unroll
            for (int j = 0; j < DB; ++j) c[j] = (cv && j < a.dim) ? a.C[(size_t)cand * a.dim + j] : 0.f;
        }
        const int cg = (a.mode == 2 && cv) ? a.group[cand] : -1;
        for (int q = 0; q < nqb; ++q) {
            const float t = rdlane(thr, q);
            float d = 0.f;
            if (DB > 0) {
                const float* qq = qs + q * DB;
#pragma unroll
                for (int j = 0; j < DB; ++j) {
                    const float df = qq[j] - c[j];
                    d = __builtin_fmaf(df, df, d);
                }
            } else if (cv) {
                const float* qq = a.Q + (size_t)(q0 + q) * a.dim;
                const float* cc = a.C + (size_t)cand * a.dim;
                for (int j = 0; j < a.dim; ++j) {
                    const float df = qq[j] - cc[j];
                    d = __builtin_fmaf(df, df, d);
                }
            }
            bool ok = cv && d < t;
            if (a.mode == 1) ok = ok && cand != q0 + q;
            else if (a.mode == 2) ok = ok && cg != rdlane(mygrp, q);
            uint64_t m = __ballot(ok);
            if (!m) continue;
            const int kq = rdlane(myk, q);
            float* L = Ld + (size_t)q * a.kmax;
            int* I = Li + (size_t)q * a.kmax;
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const float db = rdlane(d, b);
                if (!(db < rdlane(thr, q))) continue;
                knn_insert(L, I, kq, db, base + b);
                const float nt = L[kq - 1];
                if (lane == q) thr = nt;
            }
        }
    }
    if (a.lists_lds)
        for (int e = lane; e < nqb * a.kmax; e += WAVE) { a.pd[obase + e] = Ld[e]; a.pi[obase + e] = Li[e]; }
}

// One thread per query: the rank of every entry of every split list in the union is its position in the list plus the entries of
// the other splits that precede it in (d, index) order -- lower splits hold lower indices, so they precede on equal d.  Entries of
// rank < k land in the output; the other output slots stay empty (-1, kBig).
__global__ __launch_bounds__(256) void knn_merge(KnnArgs a, int nsplit, int* out_i, float* out_d) {
    const int qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= a.nq) return;
    const int kq = knn_k(a, qi);
    int* oi = out_i + (size_t)qi * a.kmax;
    float* od = out_d + (size_t)qi * a.kmax;
    for (int s = 0; s < a.kmax; ++s) { oi[s] = -1; od[s] = kBig; }
    for (int sp = 0; sp < nsplit; ++sp) {
        const size_t o = ((size_t)sp * a.nq + qi) * a.kmax;
        for (int e = 0; e < kq; ++e) {
            const int id = a.pi[o + e];
            if (id < 0) break;
            const float d = a.pd[o + e];
            int rank = e;
            for (int sq = 0; sq < nsplit && rank < kq; ++sq) {
                if (sq == sp) continue;
                const float* L = a.pd + ((size_t)sq * a.nq + qi) * a.kmax;
                const int* I = a.pi + ((size_t)sq * a.nq + qi) * a.kmax;
                int lo = 0, hi = kq;           // first entry of list sq that does not precede (d, id)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const bool before = I[mid] >= 0 && (L[mid] < d || (L[mid] == d && sq < sp));
                    if (before) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            if (rank < kq) { oi[rank] = id; od[rank] = d; }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- k-means
// Centroids Cn [R][K][cs] (cs = DB, zero padded, or dim for DB == 0); asg [R][n].  Grid (ceil(n / 256), R).
template <int DB>
__global__ __launch_bounds__(256) void km_assign(const float* __restrict__ X, int n, int dim, const float* __restrict__ Cn, int K,
                                                 int cs, int* __restrict__ asg) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[DB > 0 ? DB : 1];
    if (DB > 0) {
#pragma unroll
        for (int j = 0; j < DB; ++j) x[j] = j < dim ? X[(size_t)i * dim + j] : 0.f;
    }
    float best = kBig;
    int bc = 0;
    for (int c = 0; c < K; ++c) {
        const float* cc = Cn + ((size_t)r * K + c) * cs;
        float d = 0.f;
        if (DB > 0) {
#pragma unroll
            for (int j = 0; j < DB; ++j) {
                const float df = x[j] - cc[j];
                d = __builtin_fmaf(df, df, d);
            }
        } else {
            for (int j = 0; j < dim; ++j) {
                const float df = X[(size_t)i * dim + j] - cc[j];
                d = __builtin_fmaf(df, df, d);
            }
        }
        if (d < best) { best = d; bc = c; }
    }
    asg[(size_t)r * n + i] = bc;
}

// Block = one wave over points [b * bp, min(n, (b + 1) * bp)) of restart r; lane l owns columns j = l, l + 64, ... of every cluster
// (zeroing, summing in point order, writing out) and lane 0 the counts, so no two lanes touch one word.  P [R][nb][K][dim] fp64,
// Cnt [R][nb][K].  LDSACC: the sums accumulate in LDS (K * dim doubles) and are copied out at the end.
template <bool LDSACC>
__global__ __launch_bounds__(WAVE) void km_accum(const float* __restrict__ X, int n, int dim, const int* __restrict__ asg, int K,
                                                 int bp, double* __restrict__ P, int* __restrict__ Cnt) {
    extern __shared__ double acc_s[];
    const int lane = threadIdx.x, b = blockIdx.x, r = blockIdx.y, nb = gridDim.x;
    const size_t pb = ((size_t)r * nb + b) * K;
    double* A = LDSACC ? acc_s : P + pb * dim;
    int* Cg = Cnt + pb;
    int* Cl = LDSACC ? reinterpret_cast<int*>(acc_s + (size_t)K * dim) : Cg;
    for (int j = lane; j < dim; j += WAVE)
        for (int c = 0; c < K; ++c) A[(size_t)c * dim + j] = 0.0;
    if (lane == 0)
        for (int c = 0; c < K; ++c) Cl[c] = 0;
    const int i0 = b * bp, i1 = min(n, i0 + bp);
    const int* ar = asg + (size_t)r * n;
    for (int i = i0; i < i1; ++i) {
        const int c = ar[i];
        for (int j = lane; j < dim; j += WAVE) A[(size_t)c * dim + j] += (double)X[(size_t)i * dim + j];
        if (lane == 0) Cl[c] += 1;
    }
    if (LDSACC) {
        for (int j = lane; j < dim; j += WAVE)
            for (int c = 0; c < K; ++c) P[(pb + c) * dim + j] = A[(size_t)c * dim + j];
        if (lane == 0)
            for (int c = 0; c < K; ++c) Cg[c] = Cl[c];
    }
}

// One thread per (r, c, j): sum the nb block partials in block order, round to fp32, divide by max(count, 1) in fp32.
__global__ __launch_bounds__(256) void km_finalize(const double* __restrict__ P, const int* __restrict__ Cnt, int R, int nb, int K,
                                                   int dim, int cs, float* __restrict__ Cn) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)R * K * dim) return;
    const int j = (int)(t % dim);
    const int c = (int)((t / dim) % K);
    const int r = (int)(t / ((size_t)dim * K));
    double s = 0.0;
    int cnt = 0;
    for (int b = 0; b < nb; ++b) {
        const size_t pb = ((size_t)r * nb + b) * K + c;
        s += P[pb * dim + j];
        cnt += Cnt[pb];
    }
    Cn[((size_t)r * K + c) * cs + j] = (float)s / (float)max(cnt, 1);
}

// ---------------------------------------------------------------------------------------------------------------- silhouette
// Samples S [stot][cs] (cs = DB zero padded, or dim), grouped by class; ranges r = 0 .. nr-1 are the classes with samples, in class
// order: class rcls[r], samples [roff[r], roff[r] + rcnt[r]).  One thread per point.
constexpr int SIL_TILE_F = 4096;          // floats of one LDS sample tile

template <int DB>
__global__ __launch_bounds__(256) void sil_kernel(const float* __restrict__ X, int n, int dim, const int* __restrict__ labels,
                                                  const float* __restrict__ S, int stot, int cs, const int* __restrict__ rcls,
                                                  const int* __restrict__ roff, const int* __restrict__ rcnt, int nr,
                                                  float* __restrict__ out) {
    __shared__ float ts[DB > 0 ? SIL_TILE_F : 1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    float x[DB > 0 ? DB : 1];
    if (DB > 0) {
#pragma unroll
        for (int j = 0; j < DB; ++j) x[j] = (valid && j < dim) ? X[(size_t)i * dim + j] : 0.f;
    }
    const int my = valid ? labels[i] : -1;
    float acc = 0.f, a = 0.f, bmin = kBig;
    bool has_a = false;
    int r = 0;
    int rend = nr > 0 ? roff[0] + rcnt[0] : -1;
    auto close_range = [&](int s) {
        if (s != rend - 1) return;
        const float mean = acc / (float)rcnt[r];
        if (rcls[r] == my) { a = mean; has_a = true; }
        else if (mean < bmin) bmin = mean;
        acc = 0.f;
        ++r;
        if (r < nr) rend = roff[r] + rcnt[r];
    };
    if (DB > 0) {
        constexpr int TS = SIL_TILE_F / (DB > 0 ? DB : 1);
        for (int t0 = 0; t0 < stot; t0 += TS) {
            const int tn = min(TS, stot - t0);
            __syncthreads();
            for (int e = threadIdx.x; e < tn * DB; e += blockDim.x) ts[e] = S[(size_t)t0 * DB + e];
            __syncthreads();
            for (int s = 0; s < tn; ++s) {
                const float* sp = ts + s * DB;
                float d = 0.f;
#pragma unroll
                for (int j = 0; j < DB; ++j) {
                    const float df = x[j] - sp[j];
                    d = __builtin_fmaf(df, df, d);
                }
                acc += __builtin_sqrtf(fmaxf(d, 0.f));
                close_range(t0 + s);
            }
        }
    } else if (valid) {
        for (int s = 0; s < stot; ++s) {
            const float* sp = S + (size_t)s * cs;
            float d = 0.f;
            for (int j = 0; j < dim; ++j) {
                const float df = X[(size_t)i * dim + j] - sp[j];
                d = __builtin_fmaf(df, df, d);
            }
            acc += __builtin_sqrtf(fmaxf(d, 0.f));
            close_range(s);
        }
    }
    if (!valid) return;
    const float ai = has_a ? a : 0.f;
    const float den = fmaxf(ai, bmin);
    out[i] = den > 0.f ? (bmin - ai) / den : 0.f;
}

}  // namespace ras
