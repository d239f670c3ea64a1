// ops_cluster.hip -- bipartition() and dclust() on the device (kernels: kernels_cluster.hip.h), and their plugin entries:
// rcppml_gpu_bipartition_double / rcppml_gpu_dclust_double (the reference plugin's signatures, src/gpu_bridge_cluster.cu:57-62 and
// :105-110, with R's buffer sizes, R/bipartition.R:105-108) and the build-defined _ex forms of the Python surface.
//
// Semantics are the reference's CPU path (inst/include/FactorNet/clustering/bipartition.hpp, dclust.hpp): SplitMix64(seed) start,
// the same seed for every split, the closed-form rank-2 ALS with scale() after each half, 1 - Pearson(w, w_prev) as tolerance.
// A split depends only on its sample set and the parameters, so every split of one tree level runs TOGETHER: the CSC is uploaded
// once, each cluster is a contiguous stretch of a device permutation `perm`, and per level the clusters' columns are gathered into
// one level CSC, transposed once, and iterated by four launches per ALS iteration for all of them.
//
// Host round trips per level chunk: the transpose (it reads the level's nonzero count), the run count, one poll of the "any cluster
// still active" flag every kPoll iterations, and the read of sizes / distances / iteration counts that decides the splits.
#include "entry_common.hip.h"
#include "kernels_cluster.hip.h"

#include <climits>

namespace {
using namespace rcl;

// Polling interval: the host reads one flag (set by every cluster that stays active in the window's LAST iteration) every kPoll
// iterations.  Frozen clusters cost an early-exiting workgroup per launch, so a window that overshoots convergence wastes at most
// kPoll - 1 rounds of four near-empty launches (a few microseconds each), while a poll costs a full host round trip.
constexpr int kPoll = 8;

// Per-cluster device memory: W and the right-hand-side accumulator Wb, 2 x m doubles each.  A level whose clusters exceed the budget
// runs in chunks; every cluster is independent of the others, so the answer does not depend on the chunking.
// RCPPML_GPU_CLUSTER_BUDGET (bytes) lowers it (the tests force chunks of one or two clusters with it).
size_t cluster_budget() {
    size_t b = (size_t)2 << 30;
    if (const char* e = getenv("RCPPML_GPU_CLUSTER_BUDGET")) {
        const long long v = atoll(e);
        if (v > 0) b = (size_t)v;
    }
    return b;
}

struct Args {
    int m, n;
    int64_t nnz;
    const int* p; const int* i; const double* x;
    int maxit; double tol; int nonneg; unsigned seed;
};

void check_common(const Args& a) {
    if (a.m < 1 || a.n < 1) throw std::invalid_argument("the matrix must have at least one row and one column");
    check_csc_lenient(a.p, a.i, a.x, a.m, a.n, a.nnz);
    if (a.maxit < 1) throw std::invalid_argument("maxit must be at least 1 (the reference reads an uninitialised h at maxit = 0)");
    if (!(a.tol < 1.0)) throw std::invalid_argument("tol must be below 1 (at tol >= 1 the reference runs no iteration)");
}
unsigned seed_of(double s) {
    if (!(s >= 0.0 && s <= 4294967295.0)) throw std::invalid_argument("seed must be in [0, 2^32)");
    return static_cast<unsigned>(s);
}

// One call's device state: A uploaded once, perm, and level buffers sized for the largest level.
struct Engine {
    CtxGuard& g;
    hipStream_t s;
    Args a;
    int G;                                   // lanes per run of the row passes: a property of A alone, so that no level or chunk
                                             // choice changes a reduction order
    DevBuf dAp, dAi, dAx, dperm, dw0;
    DevBuf seg, poff, col_of, clu_of, lp, li, lx, tp, ti, tx, rcnt, rstart, rrow, rclu, h, v, side, term, W, Wb, cl, ci, any;
    int64_t nnz_cap;
    // the current chunk
    int C = 0, ncols = 0, nruns = 0;

    Engine(CtxGuard& g_, const Args& a_, const std::vector<int>& perm, int64_t nnz_cap_) : g(g_), s(g_.s), a(a_), nnz_cap(nnz_cap_) {
        const double avg = (double)a.nnz / (double)a.m;
        G = avg >= 192 ? 64 : avg >= 24 ? 16 : 4;
        upload_ints(a.p, (size_t)a.n + 1, dAp, s);
        upload_ints(a.i, (size_t)std::max<int64_t>(a.nnz, 1), dAi, s);
        upload_cast<double>(g.c, a.x, (size_t)std::max<int64_t>(a.nnz, 1), dAx, s);
        upload_ints(perm.data(), perm.size(), dperm, s);
        // the reference's initial w (bipartition.hpp:429-435): 2 x m uniform() draws of SplitMix64(seed), seed 0 -> 12345, row 0 first
        const std::vector<double> w0 = splitmix<double>(a.seed == 0 ? 12345ull : (uint64_t)a.seed, 0, (size_t)2 * a.m);
        upload_cast<double>(g.c, w0.data(), w0.size(), dw0, s);
        grow<int>(any, 1);
    }
    template <class F> void by_runs(F launch) {
        if (nruns == 0) return;
        if (G == 64) launch(std::integral_constant<int, 64>());
        else if (G == 16) launch(std::integral_constant<int, 16>());
        else launch(std::integral_constant<int, 4>());
    }
    // gather the clusters (sizes, offsets into perm) into the level CSC, transpose it, cut the CSR into runs; planes = doubles of
    // per-cluster state per row (2: W and Wb hold 2 x m each; 1: leaf centroids)
    void setup(const std::vector<int>& sizes, const std::vector<int>& offs, int planes) {
        C = (int)sizes.size();
        std::vector<int> sg(C + 1, 0);
        for (int c = 0; c < C; ++c) sg[c + 1] = sg[c] + sizes[c];
        ncols = sg[C];
        upload_ints(sg.data(), sg.size(), seg, s);
        upload_ints(offs.data(), offs.size(), poff, s);
        int* dcol = grow<int>(col_of, ncols);
        int* dclu = grow<int>(clu_of, ncols);
        int* dlp = grow<int>(lp, (size_t)ncols + 1);
        hipLaunchKernelGGL(level_cols_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), poff.as<int>(), dperm.as<int>(), dAp.as<int>(),
                           dcol, dclu, dlp);
        HIPCHK(hipMemsetAsync(dlp + ncols, 0, sizeof(int), s));
        rk::exclusive_scan_i32(g.c, dlp, dlp, (int64_t)ncols + 1);
        int* dli = grow<int>(li, (size_t)std::max<int64_t>(nnz_cap, 1));
        double* dlx = grow<double>(lx, (size_t)std::max<int64_t>(nnz_cap, 1));
        hipLaunchKernelGGL(level_gather_kernel, dim3((ncols + 3) / 4), dim3(WG), 0, s, dAp.as<int>(), dAi.as<int>(), dAx.as<double>(),
                           dcol, dlp, ncols, dli, dlx);
        HIPCHK(hipGetLastError());
        int* dtp = grow<int>(tp, (size_t)a.m + 1);
        int* dti = grow<int>(ti, (size_t)std::max<int64_t>(nnz_cap, 1));
        double* dtx = grow<double>(tx, (size_t)std::max<int64_t>(nnz_cap, 1));
        OPCHK(rcppml_hip_transpose_csc(g.c, RCPPML_F64, a.m, ncols, dlp, dli, dlx, dtp, dti, dtx));
        int* dr = grow<int>(rcnt, (size_t)a.m + 1);
        const int rb = (a.m + WG - 1) / WG;
        hipLaunchKernelGGL(run_count_kernel, dim3(rb), dim3(WG), 0, s, dtp, dti, dclu, a.m, dr);
        HIPCHK(hipMemsetAsync(dr + a.m, 0, sizeof(int), s));
        rk::exclusive_scan_i32(g.c, dr, dr, (int64_t)a.m + 1);
        int lnnz = 0;
        HIPCHK(hipMemcpyAsync(&nruns, dr + a.m, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&lnnz, dtp + a.m, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        int* drs = grow<int>(rstart, (size_t)nruns + 1);
        int* drr = grow<int>(rrow, (size_t)std::max(nruns, 1));
        int* drc = grow<int>(rclu, (size_t)std::max(nruns, 1));
        hipLaunchKernelGGL(run_fill_kernel, dim3(rb), dim3(WG), 0, s, dtp, dti, dclu, a.m, dr, drs, drr, drc, nruns, lnnz);
        grow<double>(W, (size_t)C * planes * a.m);
        grow<double>(Wb, (size_t)C * planes * a.m);
        grow<double>(cl, (size_t)C * CL_STRIDE);
        grow<int>(ci, (size_t)C * CI_STRIDE);
        grow<double>(h, (size_t)2 * ncols);
        grow<double>(v, ncols);
        grow<int>(side, ncols);
        grow<double>(term, ncols);
        HIPCHK(hipGetLastError());
    }
    // the rank-2 ALS of every cluster of the chunk, then the split (perm rewritten in place) and, with calc_dist, centers + dist
    void bipartition_all(int calc_dist) {
        const int m = a.m;
        hipLaunchKernelGGL(init_kernel, dim3(C), dim3(WG), 0, s, dw0.as<double>(), m, W.as<double>(), Wb.as<double>(), cl.as<double>(),
                           ci.as<int>());
        const int hb = (ncols + 3) / 4;
        for (int done = 0; done < a.maxit;) {
            const int P = std::min(kPoll, a.maxit - done);
            for (int k = 0; k < P; ++k) {
                if (k == P - 1) HIPCHK(hipMemsetAsync(any.p, 0, sizeof(int), s));
                hipLaunchKernelGGL(h_update_kernel, dim3(hb), dim3(WG), 0, s, lp.as<int>(), li.as<int>(), lx.as<double>(), clu_of.as<int>(),
                                   ncols, m, W.as<double>(), cl.as<double>(), ci.as<int>(), a.nonneg, h.as<double>());
                hipLaunchKernelGGL(h_scale_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), ncols, h.as<double>(), cl.as<double>(), ci.as<int>());
                by_runs([&](auto gc) {
                    constexpr int GG = decltype(gc)::value;
                    hipLaunchKernelGGL(w_rhs_kernel<GG>, dim3((nruns + WG / GG - 1) / (WG / GG)), dim3(WG), 0, s, rstart.as<int>(),
                                       rrow.as<int>(), rclu.as<int>(), nruns, ti.as<int>(), tx.as<double>(), h.as<double>(), ncols, m,
                                       ci.as<int>(), Wb.as<double>());
                });
                hipLaunchKernelGGL(w_finish_kernel, dim3(C), dim3(WG), 0, s, m, W.as<double>(), Wb.as<double>(), cl.as<double>(), ci.as<int>(),
                                   a.nonneg, a.maxit, a.tol, any.as<int>());
            }
            HIPCHK(hipGetLastError());
            done += P;
            int any_h = 0;
            HIPCHK(hipMemcpyAsync(&any_h, any.p, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (!any_h) break;
        }
        const int cb = (ncols + WG - 1) / WG;
        hipLaunchKernelGGL(orient_kernel, dim3(cb), dim3(WG), 0, s, clu_of.as<int>(), ncols, h.as<double>(), cl.as<double>(), v.as<double>(),
                           side.as<int>());
        hipLaunchKernelGGL(partition_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), poff.as<int>(), col_of.as<int>(), side.as<int>(),
                           dperm.as<int>(), ci.as<int>());
        if (calc_dist) {
            by_runs([&](auto gc) {
                constexpr int GG = decltype(gc)::value;
                hipLaunchKernelGGL(centroid_rows_kernel<GG>, dim3((nruns + WG / GG - 1) / (WG / GG)), dim3(WG), 0, s, rstart.as<int>(),
                                   rrow.as<int>(), rclu.as<int>(), nruns, ti.as<int>(), tx.as<double>(), side.as<int>(), m, 2, Wb.as<double>());
            });
            hipLaunchKernelGGL(center_finish_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), m, W.as<double>(), Wb.as<double>(),
                               cl.as<double>(), ci.as<int>());
            hipLaunchKernelGGL(relcos_kernel, dim3(hb), dim3(WG), 0, s, lp.as<int>(), li.as<int>(), lx.as<double>(), clu_of.as<int>(),
                               side.as<int>(), ncols, m, W.as<double>(), cl.as<double>(), term.as<double>());
            hipLaunchKernelGGL(dist_finish_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), side.as<int>(), term.as<double>(), m, cl.as<double>());
        }
        HIPCHK(hipGetLastError());
    }
    void read_state(std::vector<double>& clh, std::vector<int>& cih) {
        clh.resize((size_t)C * CL_STRIDE);
        cih.resize((size_t)C * CI_STRIDE);
        HIPCHK(hipMemcpyAsync(clh.data(), cl.p, clh.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cih.data(), ci.p, cih.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    // leaf centers (compute_centroid) of the clusters of the current chunk (set up with planes = 1) into host out (C x m)
    void leaf_centers(double* out) {
        HIPCHK(hipMemsetAsync(Wb.p, 0, (size_t)C * a.m * sizeof(double), s));
        by_runs([&](auto gc) {
            constexpr int GG = decltype(gc)::value;
            hipLaunchKernelGGL(centroid_rows_kernel<GG>, dim3((nruns + WG / GG - 1) / (WG / GG)), dim3(WG), 0, s, rstart.as<int>(),
                               rrow.as<int>(), rclu.as<int>(), nruns, ti.as<int>(), tx.as<double>(), (const int*)nullptr, a.m, 1,
                               Wb.as<double>());
        });
        hipLaunchKernelGGL(leaf_center_kernel, dim3(C), dim3(WG), 0, s, seg.as<int>(), a.m, Wb.as<double>(), W.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out, W.p, (size_t)C * a.m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    std::vector<int> perm_host(size_t count) {
        std::vector<int> p(count);
        HIPCHK(hipMemcpyAsync(p.data(), dperm.p, count * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return p;
    }
};

size_t chunk_clusters(int m, int planes) {
    const size_t per = (size_t)planes * 2 * (size_t)m * sizeof(double);
    return std::max<size_t>(1, cluster_budget() / per);
}

// ------------------------------------------------------------------------------------------------------------ bipartition
struct BipResult {
    std::vector<double> v, center;          // v: n_sub; center: 2 m (zeros without calc_dist)
    std::vector<int> side;                  // 1 = samples1
    int size1 = 0, size2 = 0, iter = 0;
    double dist = -1;
};

BipResult bipartition_run(const Args& a, const std::vector<int>& samples, int calc_dist) {
    check_common(a);
    const int ns = (int)samples.size();
    if (ns < 1) throw std::invalid_argument("samples must not be empty");
    int64_t cap = 0;
    for (int j : samples) {
        if (j < 0 || j >= a.n) throw std::invalid_argument("sample index out of range");
        cap += a.p[j + 1] - a.p[j];
    }
    if (cap >= INT_MAX) throw std::invalid_argument("the sample subset holds more than 2^31 nonzeros");
    CtxGuard g(env_device());
    Engine E(g, a, samples, cap);
    E.setup({ns}, {0}, 2);
    E.bipartition_all(calc_dist);
    BipResult r;
    r.v.resize(ns); r.side.resize(ns); r.center.assign((size_t)2 * a.m, 0.0);
    HIPCHK(hipMemcpyAsync(r.v.data(), E.v.p, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, E.s));
    HIPCHK(hipMemcpyAsync(r.side.data(), E.side.p, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, E.s));
    if (calc_dist) HIPCHK(hipMemcpyAsync(r.center.data(), E.W.p, (size_t)2 * a.m * sizeof(double), hipMemcpyDeviceToHost, E.s));
    std::vector<double> clh; std::vector<int> cih;
    E.read_state(clh, cih);
    r.size1 = cih[CI_SIZE1]; r.size2 = ns - r.size1; r.iter = cih[CI_ITER];
    r.dist = calc_dist ? clh[CL_DIST] : -1.0;
    return r;
}

// ------------------------------------------------------------------------------------------------------------ dclust
struct Node { int parent, bit, off, size, iter = -1, child0 = -1; double radius = 0; };
struct Tree {
    std::vector<Node> nodes;
    std::vector<int> leaves;                // node ids in the CPU's emission order (dclust.hpp: LIFO, "1" child popped first)
    std::vector<int> perm;                  // leaves are contiguous stretches of it
    std::vector<double> centers;            // leaves x m, emission order (when asked for)
};

Tree dclust_run(const Args& a, int min_samples, double min_dist, bool want_centers) {
    check_common(a);
    if (min_samples < 1) throw std::invalid_argument("min_samples must be at least 1 (the reference never terminates at 0)");
    const bool calc_dist = min_dist > 0;
    std::vector<int> perm(a.n);
    std::iota(perm.begin(), perm.end(), 0);
    CtxGuard g(env_device());
    Engine E(g, a, perm, a.nnz);
    Tree T;
    T.nodes.push_back(Node{-1, -1, 0, a.n});
    std::vector<int> pending{0};
    const size_t chunk = chunk_clusters(a.m, 2);
    while (!pending.empty()) {
        std::vector<int> split;
        for (int id : pending)
            if (T.nodes[id].size >= 2 * min_samples) split.push_back(id);      // smaller: a leaf (radius 0)
        std::vector<int> next;
        for (size_t c0 = 0; c0 < split.size(); c0 += chunk) {
            const size_t c1 = std::min(split.size(), c0 + chunk);
            std::vector<int> sizes, offs;
            for (size_t k = c0; k < c1; ++k) { sizes.push_back(T.nodes[split[k]].size); offs.push_back(T.nodes[split[k]].off); }
            E.setup(sizes, offs, 2);
            E.bipartition_all(calc_dist);
            std::vector<double> clh; std::vector<int> cih;
            E.read_state(clh, cih);
            for (size_t k = c0; k < c1; ++k) {
                const size_t c = k - c0;
                const int id = split[k];
                const int s1 = cih[c * CI_STRIDE + CI_SIZE1], s2 = T.nodes[id].size - s1;
                const double dist = clh[c * CL_STRIDE + CL_DIST];
                T.nodes[id].iter = cih[c * CI_STRIDE + CI_ITER];
                bool ok = s1 >= min_samples && s2 >= min_samples;
                if (ok && calc_dist && dist < min_dist) ok = false;           // NaN dist passes, as on the CPU
                if (ok) {
                    const Node n = T.nodes[id];
                    T.nodes[id].child0 = (int)T.nodes.size();
                    T.nodes.push_back(Node{id, 0, n.off, s1});
                    T.nodes.push_back(Node{id, 1, n.off + s1, s2});
                    next.push_back(T.nodes[id].child0);
                    next.push_back(T.nodes[id].child0 + 1);
                } else {
                    T.nodes[id].radius = calc_dist ? dist : 0.0;
                }
            }
        }
        pending.swap(next);
    }
    // emission order
    std::vector<int> stack{0};
    while (!stack.empty()) {
        const int id = stack.back();
        stack.pop_back();
        if (T.nodes[id].child0 < 0) { T.leaves.push_back(id); continue; }
        stack.push_back(T.nodes[id].child0);
        stack.push_back(T.nodes[id].child0 + 1);
    }
    T.perm = E.perm_host(a.n);
    if (want_centers) {
        const int L = (int)T.leaves.size();
        T.centers.resize((size_t)L * a.m);
        const size_t lchunk = chunk_clusters(a.m, 1);             // one plane of m doubles per leaf in W and in Wb
        for (size_t c0 = 0; c0 < (size_t)L; c0 += lchunk) {
            const size_t c1 = std::min((size_t)L, c0 + lchunk);
            std::vector<int> sizes, offs;
            for (size_t k = c0; k < c1; ++k) { sizes.push_back(T.nodes[T.leaves[k]].size); offs.push_back(T.nodes[T.leaves[k]].off); }
            E.setup(sizes, offs, 1);
            E.leaf_centers(T.centers.data() + c0 * (size_t)a.m);
        }
    }
    return T;
}

Args make_args(const int* col_ptr, const int* row_idx, const double* values, const int* m, const int* n, const int* nnz,
               const int* max_iter, const double* tol, const int* nonneg, const double* seed) {
    Args a;
    a.m = *m; a.n = *n; a.nnz = *nnz; a.p = col_ptr; a.i = row_idx; a.x = values;
    a.maxit = *max_iter; a.tol = *tol; a.nonneg = *nonneg != 0; a.seed = seed_of(*seed);
    return a;
}

// capacity check of a build-defined output: *len holds the capacity on input; too small -> refuse, report the size needed
void need(int* len, int64_t needed, const char* what) {
    if (!len) throw std::invalid_argument(std::string(what) + ": capacity pointer is NULL");
    if ((int64_t)*len < needed) {
        const int cap = *len;
        *len = (int)needed;
        throw std::invalid_argument(std::string(what) + " holds " + std::to_string(cap) + " entries, " + std::to_string(needed) +
                                    " are needed");
    }
}

}  // namespace

extern "C" void rcppml_gpu_bipartition_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                              int* max_iter, double* tol, int* nonneg, double* seed, int* partition, double* v,
                                              double* center, double* dist, int* out_status) {
    entry_guard(out_status, [&] {
        const Args a = make_args(col_ptr, row_idx, values, m, n, nnz, max_iter, tol, nonneg, seed);
        std::vector<int> all(std::max(*n, 0));
        std::iota(all.begin(), all.end(), 0);
        const BipResult r = bipartition_run(a, all, 1);
        // R's buffers (R/bipartition.R:105-108): partition n ints (0 = samples1, as R reads it back), v m doubles (the first
        // min(m, n) scores, as the reference bridge writes), center 2 m doubles
        for (int j = 0; j < a.n; ++j) partition[j] = r.side[j] ? 0 : 1;
        for (int j = 0; j < std::min(a.m, a.n); ++j) v[j] = r.v[j];
        std::copy(r.center.begin(), r.center.end(), center);
        *dist = r.dist;
    });
}

extern "C" void rcppml_gpu_bipartition_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                          const int* samples, int* n_samples, int* max_iter, double* tol, int* nonneg, double* seed,
                                          int* calc_dist, int* partition, int* partition_len, double* v, int* v_len, double* center,
                                          int* center_len, int* out_size1, int* out_size2, double* out_dist, int* out_iter,
                                          int* out_status) {
    entry_guard(out_status, [&] {
        const Args a = make_args(col_ptr, row_idx, values, m, n, nnz, max_iter, tol, nonneg, seed);
        std::vector<int> smp;
        if (samples && *n_samples > 0) smp.assign(samples, samples + *n_samples);
        else { smp.resize(std::max(*n, 0)); std::iota(smp.begin(), smp.end(), 0); }
        const int64_t ns = (int64_t)smp.size();
        need(partition_len, ns, "partition");
        need(v_len, ns, "v");
        need(center_len, (int64_t)2 * a.m, "center");
        const BipResult r = bipartition_run(a, smp, *calc_dist != 0);
        for (int64_t j = 0; j < ns; ++j) { partition[j] = r.side[j] ? 0 : 1; v[j] = r.v[j]; }
        std::copy(r.center.begin(), r.center.end(), center);
        *partition_len = (int)ns; *v_len = (int)ns; *center_len = 2 * a.m;
        *out_size1 = r.size1; *out_size2 = r.size2; *out_dist = r.dist; *out_iter = r.iter;
    });
}

extern "C" void rcppml_gpu_dclust_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                         int* max_clusters, int* min_samples, double* min_dist, int* max_iter, double* tol, int* nonneg,
                                         double* seed, int* assignments, int* out_num_clusters, int* out_status) {
    entry_guard(out_status, [&] {
        const Args a = make_args(col_ptr, row_idx, values, m, n, nnz, max_iter, tol, nonneg, seed);
        const Tree T = dclust_run(a, *min_samples, *min_dist, false);
        int nc = (int)T.leaves.size();
        if (*max_clusters > 0 && nc > *max_clusters) nc = *max_clusters;     // later clusters: -1, as the reference bridge
        for (int j = 0; j < a.n; ++j) assignments[j] = -1;
        for (int c = 0; c < nc; ++c) {
            const Node& L = T.nodes[T.leaves[c]];
            for (int k = L.off; k < L.off + L.size; ++k) assignments[T.perm[k]] = c;
        }
        *out_num_clusters = nc;
    });
}

extern "C" void rcppml_gpu_dclust_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                     int* min_samples, double* min_dist, int* max_iter, double* tol, int* nonneg, double* seed,
                                     int* assignments, int* cluster_cap, int* out_size, double* out_radius, int* out_node,
                                     double* out_center, int* node_cap, int* node_parent, int* node_bit, int* node_iter,
                                     int* out_status) {
    entry_guard(out_status, [&] {
        const Args a = make_args(col_ptr, row_idx, values, m, n, nnz, max_iter, tol, nonneg, seed);
        if (!cluster_cap || !node_cap) throw std::invalid_argument("capacity pointer is NULL");
        const Tree T = dclust_run(a, *min_samples, *min_dist, out_center != nullptr);
        const int L = (int)T.leaves.size(), N = (int)T.nodes.size();
        need(cluster_cap, L, "cluster outputs");
        need(node_cap, N, "split tree");
        for (int j = 0; j < a.n; ++j) assignments[j] = -1;
        for (int c = 0; c < L; ++c) {
            const Node& nd = T.nodes[T.leaves[c]];
            for (int k = nd.off; k < nd.off + nd.size; ++k) assignments[T.perm[k]] = c;
            out_size[c] = nd.size; out_radius[c] = nd.radius; out_node[c] = T.leaves[c];
        }
        for (int k = 0; k < N; ++k) { node_parent[k] = T.nodes[k].parent; node_bit[k] = T.nodes[k].bit; node_iter[k] = T.nodes[k].iter; }
        if (out_center) std::copy(T.centers.begin(), T.centers.end(), out_center);
        *cluster_cap = L; *node_cap = N;
    });
}
