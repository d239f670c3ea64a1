// ops_consensus.hip -- consensus clustering: the stage of the reference's consensus_nmf that follows the fits (R/consensus.R:102-137).
// rcppml_gpu_consensus_double builds the m x m consensus matrix from the stacked loadings on the device (kernels:
// kernels_consensus.hip.h); rcppml_gpu_hclust_average_double is hclust(as.dist(d), "average"), cutree and the cophenetic correlation
// in host C++ (no device is touched, so it runs on a machine without one).  Both are build-defined: R has no hook for them.
//
// knn_jaccard works a replicate at a time: sim = Wn Wn^T is formed a strip of rows at a time into a scratch of at most kStripBytes
// (never the whole m x m unless it is that small), each row's actual_k-th largest similarity is found exactly by bisection over the
// strip, the neighbour sets become bitsets, and J is added into the result in replicate order.  The selection reads a row many
// times, which is why the strip is written rather than kept in registers: LDS cannot hold a row for every m, and actual_k can be
// anything up to m - 1.
//
// Rules where the reference is undefined: equal similarities go to the lower index; a zero-norm row has similarity 0 to everything.
// Tree ties: among equal smallest dissimilarities the pair with the smallest lower index, then the smallest upper index, is merged
// (believed to be what R's hclust does; not verified against R).
#include "entry_common.hip.h"
#include "kernels_consensus.hip.h"

#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace {
using namespace rcppml_plugin;
using namespace rcons;

constexpr size_t kStripBytes = size_t(64) << 20;     // sim strip scratch

unsigned blocks(int64_t n, int per) {
    const int64_t b = (n + per - 1) / per;
    if (b >= ((int64_t)1 << 31)) throw std::invalid_argument("the call is too large for one launch grid");
    return (unsigned)b;
}

// ------------------------------------------------------------------------------------------------------------ average linkage
// Lance-Williams with the operations in this order, unfused (the restatement in the tests does the same arithmetic)
inline double lw_average(double na, double da, double nb, double db) {
#pragma clang fp contract(off)
    return (na * da + nb * db) / (na + nb);
}

struct Tree {
    std::vector<int> merge;          // (m - 1) x 2, column-major, R's convention
    std::vector<double> height;
    std::vector<int> clusters;
    double cophenetic = 0;
};

// dist: m x m column-major, entries (i, j) with i > j read.  The work matrix holds d(i, j) at D[min * m + max] (row = lower index).
Tree hclust_average(const double* dist, int64_t m, int k_cut) {
    Tree t;
    t.merge.assign((size_t)(2 * (m - 1)), 0);
    t.height.assign((size_t)(m - 1), 0.0);
    std::vector<double> D((size_t)(m * m), 0.0);
    for (int64_t j = 0; j < m; ++j)
        for (int64_t i = j + 1; i < m; ++i) D[(size_t)(j * m + i)] = dist[(size_t)(j * m + i)];
    auto d = [&](int64_t a, int64_t b) -> double& { return a < b ? D[(size_t)(a * m + b)] : D[(size_t)(b * m + a)]; };
    std::vector<char> active((size_t)m, 1);
    std::vector<int64_t> nn((size_t)m, -1), size((size_t)m, 1);
    std::vector<double> dnn((size_t)m, 0.0);
    std::vector<int> id((size_t)m);                       // R's name of the cluster in a slot: -(i + 1) or the step that made it
    for (int64_t i = 0; i < m; ++i) id[(size_t)i] = -(int)(i + 1);
    // nn[i]: the first smallest d(i, j) over active j > i
    auto rescan = [&](int64_t i) {
        nn[(size_t)i] = -1;
        for (int64_t j = i + 1; j < m; ++j)
            if (active[(size_t)j] && (nn[(size_t)i] < 0 || D[(size_t)(i * m + j)] < dnn[(size_t)i])) {
                nn[(size_t)i] = j;
                dnn[(size_t)i] = D[(size_t)(i * m + j)];
            }
    };
    for (int64_t i = 0; i + 1 < m; ++i) rescan(i);

    // the Pearson sums need the means first: x = the input dissimilarities, y = the cophenetic distances (a merge of clusters of
    // sizes p and q at height h gives p * q pairs the distance h)
    const double npairs = (double)m * (double)(m - 1) / 2.0;
    double sx = 0, xmin = std::numeric_limits<double>::infinity(), xmax = -xmin;
    for (int64_t j = 0; j < m; ++j)
        for (int64_t i = j + 1; i < m; ++i) {
            const double v = dist[(size_t)(j * m + i)];
            sx += v;
            xmin = std::min(xmin, v);
            xmax = std::max(xmax, v);
        }
    struct Step { int64_t a, b; };
    std::vector<Step> steps((size_t)(m - 1));
    double sy = 0;
    for (int64_t s = 0; s + 1 < m; ++s) {
        int64_t a = -1;
        for (int64_t i = 0; i < m; ++i)
            if (active[(size_t)i] && nn[(size_t)i] >= 0 && (a < 0 || dnn[(size_t)i] < dnn[(size_t)a])) a = i;
        const int64_t b = nn[(size_t)a];
        const double h = dnn[(size_t)a];
        const int ia = id[(size_t)a], ib = id[(size_t)b];
        // singletons before clusters; two singletons: the lower sample first; two clusters: the earlier step first
        int first = ia, second = ib;
        if ((ia < 0 && ib < 0) ? (ia < ib) : (ia > 0 && ib > 0) ? (ia > ib) : (ia > 0)) std::swap(first, second);
        t.merge[(size_t)s] = first;
        t.merge[(size_t)(m - 1 + s)] = second;
        t.height[(size_t)s] = h;
        sy += h * (double)size[(size_t)a] * (double)size[(size_t)b];
        steps[(size_t)s].a = a; steps[(size_t)s].b = b;
        // the merged cluster keeps slot a
        const double na = (double)size[(size_t)a], nb = (double)size[(size_t)b];
        active[(size_t)b] = 0;
        nn[(size_t)b] = -1;
        for (int64_t c = 0; c < m; ++c)
            if (active[(size_t)c] && c != a) d(a, c) = lw_average(na, d(a, c), nb, d(b, c));
        size[(size_t)a] += size[(size_t)b];
        id[(size_t)a] = (int)(s + 1);
        for (int64_t c = 0; c < m; ++c) {
            if (!active[(size_t)c] || c == a || nn[(size_t)c] < 0) continue;
            if (nn[(size_t)c] == a || nn[(size_t)c] == b) rescan(c);
            else if (c < a) {
                const double v = D[(size_t)(c * m + a)];
                if (v < dnn[(size_t)c] || (v == dnn[(size_t)c] && a < nn[(size_t)c])) { nn[(size_t)c] = a; dnn[(size_t)c] = v; }
            }
        }
        rescan(a);
    }
    // cutree: the first m - k_cut merges stand; clusters numbered by first appearance
    std::vector<int> parent((size_t)m);
    for (int64_t i = 0; i < m; ++i) parent[(size_t)i] = (int)i;
    for (int64_t s = 0; s < m - k_cut; ++s) parent[(size_t)steps[(size_t)s].b] = (int)steps[(size_t)s].a;
    std::vector<int> number((size_t)m, 0);
    t.clusters.assign((size_t)m, 0);
    int next = 0;
    for (int64_t i = 0; i < m; ++i) {
        int r = (int)i;
        while (parent[(size_t)r] != r) r = parent[(size_t)r];
        if (!number[(size_t)r]) number[(size_t)r] = ++next;
        t.clusters[(size_t)i] = number[(size_t)r];
    }
    // Pearson correlation, two passes (the second replays the merges to list the pairs each one joins); clamped as R's cor does
    const double mx = sx / npairs, my = sy / npairs;
    double hmin = t.height[0], hmax = t.height[0];
    for (double h : t.height) { hmin = std::min(hmin, h); hmax = std::max(hmax, h); }
    if (xmin == xmax || hmin == hmax) {
        t.cophenetic = std::numeric_limits<double>::quiet_NaN();
        return t;
    }
    std::vector<std::vector<int>> members((size_t)m);
    for (int64_t i = 0; i < m; ++i) members[(size_t)i].assign(1, (int)i);
    double sxx = 0, syy = 0, sxy = 0;
    for (int64_t s = 0; s + 1 < m; ++s) {
        std::vector<int>& ma = members[(size_t)steps[(size_t)s].a];
        std::vector<int>& mb = members[(size_t)steps[(size_t)s].b];
        const double dy = t.height[(size_t)s] - my;
        for (int u : ma)
            for (int v : mb) {
                const double dx = dist[(size_t)(u < v ? (int64_t)u * m + v : (int64_t)v * m + u)] - mx;
                sxx += dx * dx;
                sxy += dx * dy;
            }
        syy += dy * dy * (double)ma.size() * (double)mb.size();
        ma.insert(ma.end(), mb.begin(), mb.end());
        std::vector<int>().swap(mb);
    }
    t.cophenetic = std::max(-1.0, std::min(1.0, sxy / std::sqrt(sxx * syy)));
    return t;
}

}  // namespace

extern "C" void rcppml_gpu_consensus_double(const double* W_stack, int* m, int* k, int* reps, int* method, int* knn,
                                            double* out_consensus, int* out_labels, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !k || !reps || !method || !knn) throw std::invalid_argument("null scalar argument");
        if (*m < 2) throw std::invalid_argument("m must be >= 2");
        if (*k < 1) throw std::invalid_argument("k must be >= 1");
        if (*reps < 1) throw std::invalid_argument("reps must be >= 1");
        if (*method != 0 && *method != 1) throw std::invalid_argument("method must be 0 (hard) or 1 (knn_jaccard)");
        if (*knn < 1) throw std::invalid_argument("knn must be >= 1");
        if (!W_stack) throw std::invalid_argument("null W_stack");
        if (!out_consensus) throw std::invalid_argument("null out_consensus");
        const int64_t M = *m, R = *reps;
        const int K = *k;
        const bool hard = *method == 0;
        const size_t nW = (size_t)R * (size_t)M * (size_t)K;
        for (size_t q = 0; q < nW; ++q)
            if (!std::isfinite(W_stack[q])) throw std::invalid_argument("W_stack holds a non-finite value");
        const int64_t words = (M + 63) / 64;
        const int64_t tiles = (M + T - 1) / T;
        if (tiles > 65535) throw std::invalid_argument("m is too large for the tile grid");
        const int actual_k = (int)std::min<int64_t>(*knn, M - 1);
        // rows of sim per strip: whole tiles, at most kStripBytes
        int64_t strip = std::max<int64_t>(T, (int64_t)(kStripBytes / (8 * (size_t)M)) / T * T);
        strip = std::min(strip, tiles * T);
        const size_t need = 8 * (size_t)M * (size_t)M + 8 * nW +
                            (hard ? 4 * (size_t)R * (size_t)M : 8 * (size_t)M * (size_t)words + 8 * (size_t)strip * (size_t)M) + 4096;
        device_ready(need);
        Stream st;
        DevBuf dW, dOut, dLab, dBits, dS;
        dW.alloc(8 * nW);
        HIPCHK(hipMemcpyAsync(dW.p, W_stack, 8 * nW, hipMemcpyHostToDevice, st.s));
        dOut.alloc(8 * (size_t)M * (size_t)M);
        const dim3 grid((unsigned)tiles, (unsigned)tiles);
        std::vector<int> lab;
        if (hard) {
            dLab.alloc(4 * (size_t)R * (size_t)M);
            hipLaunchKernelGGL(labels_kernel, dim3(blocks(R * M, NT)), dim3(NT), 0, st.s, dW.as<double>(), R * M, K, dLab.as<int>());
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(hard_tile_kernel, grid, dim3(NT), 0, st.s, dLab.as<int>(), M, (int)R, dOut.as<double>());
            HIPCHK(hipGetLastError());
            if (out_labels) {
                lab.resize((size_t)R * (size_t)M);
                HIPCHK(hipMemcpyAsync(lab.data(), dLab.p, 4 * lab.size(), hipMemcpyDeviceToHost, st.s));
            }
        } else {
            dBits.alloc(8 * (size_t)M * (size_t)words);
            dS.alloc(8 * (size_t)strip * (size_t)M);
            hipLaunchKernelGGL(normalize_kernel, dim3(blocks(R * M, NT)), dim3(NT), 0, st.s, dW.as<double>(), R * M, K);
            HIPCHK(hipGetLastError());
            for (int64_t r = 0; r < R; ++r) {
                const double* Wn = dW.as<double>() + (size_t)r * (size_t)M * (size_t)K;
                for (int64_t i0 = 0; i0 < M; i0 += strip) {
                    const int64_t nrows = std::min(strip, M - i0);
                    hipLaunchKernelGGL(sim_tile_kernel, dim3((unsigned)tiles, (unsigned)((nrows + T - 1) / T)), dim3(NT), 0, st.s, Wn, M,
                                       K, i0, nrows, dS.as<double>());
                    hipLaunchKernelGGL(select_kernel, dim3(blocks(nrows, NT / 64)), dim3(NT), 0, st.s, dS.as<double>(), M, i0, nrows,
                                       actual_k, words, dBits.as<unsigned long long>());
                }
                hipLaunchKernelGGL(jaccard_tile_kernel, grid, dim3(NT), 0, st.s, dBits.as<unsigned long long>(), M, words, actual_k,
                                   r == 0 ? 1 : 0, r == R - 1 ? 1 : 0, (double)R, dOut.as<double>());
                HIPCHK(hipGetLastError());
            }
        }
        // nothing is written to the caller's buffers before the device work has succeeded
        HIPCHK(hipStreamSynchronize(st.s));
        HIPCHK(hipMemcpy(out_consensus, dOut.p, 8 * (size_t)M * (size_t)M, hipMemcpyDeviceToHost));
        if (hard && out_labels) std::copy(lab.begin(), lab.end(), out_labels);
    });
}

extern "C" void rcppml_gpu_hclust_average_double(const double* dist, int* m, int* k_cut, int* out_merge, double* out_height,
                                                 int* out_clusters, double* out_cophenetic, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !k_cut) throw std::invalid_argument("null scalar argument");
        if (*m < 2) throw std::invalid_argument("m must be >= 2");
        if (*k_cut < 1 || *k_cut > *m) throw std::invalid_argument("k_cut must lie in [1, m]");
        if (!dist) throw std::invalid_argument("null dist");
        if (!out_merge || !out_height || !out_clusters || !out_cophenetic) throw std::invalid_argument("null output");
        const int64_t M = *m;
        for (int64_t j = 0; j < M; ++j)
            for (int64_t i = j + 1; i < M; ++i)
                if (!std::isfinite(dist[(size_t)(j * M + i)])) throw std::invalid_argument("dist holds a non-finite value");
        const Tree t = hclust_average(dist, M, *k_cut);
        std::copy(t.merge.begin(), t.merge.end(), out_merge);
        std::copy(t.height.begin(), t.height.end(), out_height);
        std::copy(t.clusters.begin(), t.clusters.end(), out_clusters);
        *out_cophenetic = t.cophenetic;
    });
}
