// ops_classify_rf.hip -- the histogram random forest on the device (kernels: kernels_classify_rf.hip.h) and its build-defined entry
// rcppml_gpu_classify_rf_ex: the device side of the reference's classify_rf (R/classifier_metrics.R:315-380), which hands the work
// to the randomForest package on the CPU.  The algorithm is the project's own (restated in tests/classify_rf_ref.py):
// 256 uniform bins per feature, bootstrap and candidate features from the counter-based SplitMix64 stream, breadth-first growth of all
// trees of a batch one level per round of launches.  Votes go through the metrics stage of ops_classify.hip.
//
// Every argument is checked before the device is touched, and outputs are written only after the last device call has returned,
// so a refused or failed call leaves every output buffer as it was.
#include "entry_common.hip.h"
#include "kernels_classify_rf.hip.h"

#include <chrono>
#include <cmath>

namespace {
using namespace rcppml_plugin;
using namespace rrf;

constexpr size_t TREE_BYTES_PER_ROW = 128;        // mult 4, entries 2 x 8, seg 32, nodes 32, work lists 2 x 8, rec 16, child 4, large 2 x 4

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class K> void search_launch(K kernel, DynSmemOnce& once, int device, int grid, size_t lds, hipStream_t s, const GrowArgs& a) {
    once.ensure(reinterpret_cast<const void*>(kernel), lds, device);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), lds, s, a);
}

}  // namespace

extern "C" void rcppml_gpu_classify_rf_ex(const double* train, const double* test, const int* train_labels, const int* test_labels,
                                          int* n_train, int* n_test, int* dim, int* n_classes, int* ntree, int* mtry, int* seed,
                                          int* tree_batch, int* out_votes, double* out_prob, int* out_predictions, int* out_confusion,
                                          double* out_precision, double* out_recall, double* out_f1, int* out_support,
                                          double* out_auc, int* out_feature, int* out_threshold, int* out_left, int* out_class,
                                          int* out_n_nodes, double* out_lo, double* out_hi, double* out_ms, int* out_launches,
                                          int* out_status) {
    entry_guard(out_status, [&] {
        if (!n_train || !n_test || !dim || !n_classes || !ntree || !mtry || !seed) throw std::invalid_argument("null scalar argument");
        if (!train || !test || !train_labels || !test_labels) throw std::invalid_argument("null array");
        const int n = *n_train, nte = *n_test, p = *dim, C = *n_classes, T = *ntree;
        if (n < 1 || nte < 1) throw std::invalid_argument("n_train and n_test must be >= 1");
        if (p < 1 || p > PMAX) throw std::invalid_argument("dim must be in [1, 128]");
        if (C < 2 || C > CMAX) throw std::invalid_argument("n_classes must be in [2, 64]");
        if (T < 1 || T > 4096) throw std::invalid_argument("ntree must be in [1, 4096]");
        if (*mtry < 0 || *mtry > p) throw std::invalid_argument("mtry must be in [1, dim] (0: floor(sqrt(dim)))");
        if (*seed < 0) throw std::invalid_argument("seed must be >= 0");
        if (tree_batch && *tree_batch < 0) throw std::invalid_argument("tree_batch must be >= 0");
        if (n > INT_MAX / 4) throw std::invalid_argument("n_train must be below 2^29");
        for (int i = 0; i < n; ++i)
            if (train_labels[i] < 0 || train_labels[i] >= C) throw std::invalid_argument("train_labels holds a label outside [0, n_classes)");
        for (int i = 0; i < nte; ++i)
            if (test_labels[i] < 0 || test_labels[i] >= C) throw std::invalid_argument("test_labels holds a label outside [0, n_classes)");
        all_finite(train, (size_t)n * p, "the training embedding");
        all_finite(test, (size_t)nte * p, "the test embedding");
        if (!out_votes || !out_prob || !out_predictions || !out_confusion || !out_precision || !out_recall || !out_f1 || !out_support ||
            !out_auc)
            throw std::invalid_argument("null output");
        const bool forest = out_feature || out_threshold || out_left || out_class || out_n_nodes || out_lo || out_hi;
        if (forest && !(out_feature && out_threshold && out_left && out_class && out_n_nodes && out_lo && out_hi))
            throw std::invalid_argument("the forest outputs are given together or not at all");
        int m = *mtry;
        if (m == 0) {
            m = (int)std::floor(std::sqrt((double)p));
            while ((m + 1) * (m + 1) <= p) ++m;
            while (m * m > p) --m;
            m = std::max(m, 1);
        }
        const uint64_t sd = *seed == 0 ? 12345ull : (uint64_t)*seed;       // the stream takes seed 0 as 12345 (rng/rng.hpp)

        const size_t fixed = (size_t)(n + nte) * p * 9 + (size_t)n + (size_t)nte * C * 4 + (size_t)p * 16 + 4096;
        const size_t per_tree = TREE_BYTES_PER_ROW * (size_t)n + 64;
        device_ready(fixed + per_tree, "the random forest");
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        // trees per batch: half of the free memory, work-list indices below 2^31, or what the caller forces (a test switch)
        size_t Bz = std::max<size_t>(1, (free_b / 2 > fixed ? free_b / 2 - fixed : 0) / per_tree);
        Bz = std::min<size_t>(Bz, (size_t)INT_MAX / (2 * (size_t)n));
        int B = (int)std::min<size_t>(std::max<size_t>(Bz, 1), (size_t)T);
        if (tree_batch && *tree_batch > 0) B = std::min(B, *tree_batch);
        const int device = env_device();

        std::vector<uint8_t> y8(n);
        for (int i = 0; i < n; ++i) y8[i] = (uint8_t)train_labels[i];
        Stream st;
        hipStream_t s = st.s;
        DevBuf Xb, Tb, Yb, Lob, Hib, Bnb, Btb, Vb;
        const double* dX = upload<double>(Xb, train, (size_t)n * p, s);
        const double* dT = upload<double>(Tb, test, (size_t)nte * p, s);
        const uint8_t* dY = upload<uint8_t>(Yb, y8.data(), n, s);
        double* dLo = dalloc<double>(Lob, p);
        double* dHi = dalloc<double>(Hib, p);
        uint8_t* dBins = dalloc<uint8_t>(Bnb, (size_t)n * p);
        uint8_t* dTbins = dalloc<uint8_t>(Btb, (size_t)nte * p);
        int* dVotes = zeros<int>(Vb, (size_t)nte * C, s);
        int launches = 0;
        std::vector<double> ms(2 + MAX_DEPTH + 1, 0.0);
        double t_mark = now_ms();
        hipLaunchKernelGGL(rf_minmax, dim3(p), dim3(THREADS), 0, s, dX, n, p, dLo, dHi);
        hipLaunchKernelGGL(rf_bin, dim3((unsigned)(((size_t)n * p + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, dX, n, p, dLo, dHi, dBins);
        hipLaunchKernelGGL(rf_bin, dim3((unsigned)(((size_t)nte * p + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, dT, nte, p, dLo, dHi,
                           dTbins);
        HIPCHK(hipGetLastError());
        launches += 3;

        const size_t Bn = (size_t)B * n;
        DevBuf Mb, E0, E1, Sb, Nb, Rb, Cb, A0, A1, O0, O1, G0, G1, Kb, Ncb, Lbb, Nsb;
        uint32_t* dMult = dalloc<uint32_t>(Mb, Bn);
        uint2* dEnt[2] = {dalloc<uint2>(E0, Bn), dalloc<uint2>(E1, Bn)};
        int2* dAct[2] = {dalloc<int2>(A0, Bn), dalloc<int2>(A1, Bn)};
        int* dOff[2] = {dalloc<int>(O0, (size_t)B + 1), dalloc<int>(O1, (size_t)B + 1)};
        int* dLarge[2] = {dalloc<int>(G0, Bn), dalloc<int>(G1, Bn)};
        GrowArgs a{};
        a.bins = dBins; a.y = dY;
        a.seg = dalloc<int4>(Sb, 2 * Bn);
        a.nodes = dalloc<int4>(Nb, 2 * Bn);
        a.rec = dalloc<int4>(Rb, Bn);
        a.child = dalloc<int>(Cb, Bn);
        a.counters = dalloc<int>(Kb, 2);
        a.ncount = dalloc<int>(Ncb, B);
        a.lvl_base = dalloc<int>(Lbb, B);
        a.nsplit = dalloc<int>(Nsb, B);
        a.n = n; a.p = p; a.C = C; a.mtry = m; a.ntree = T; a.seed = sd;

        static DynSmemOnce once_large, once_small, once_predict;
        const size_t lds_large = rf_search_lds(C, 4), lds_small = rf_search_lds(C, 1), lds_predict = (size_t)LDS_NODES * sizeof(int4);
        once_predict.ensure(reinterpret_cast<const void*>(rf_predict), lds_predict, device);

        std::vector<int4> h_nodes;
        std::vector<int> h_ncount, f_feat, f_thr, f_left, f_cls, f_nn;
        if (forest) {
            f_feat.assign((size_t)T * 2 * n, -1); f_thr = f_feat; f_left = f_feat; f_cls = f_feat;
            f_nn.assign(T, 0);
        }
        ms[0] += now_ms() - t_mark;
        for (int t0 = 0; t0 < T; t0 += B) {
            const int Bc = std::min(B, T - t0);
            t_mark = now_ms();
            a.B = Bc; a.t0 = t0;
            int cur = 0;                      // the buffers rf_root fills become those of level 0
            HIPCHK(hipMemsetAsync(dMult, 0, (size_t)Bc * n * sizeof(uint32_t), s));
            HIPCHK(hipMemsetAsync(a.counters, 0, 2 * sizeof(int), s));
            hipLaunchKernelGGL(rf_bootstrap, dim3((n + THREADS - 1) / THREADS, Bc), dim3(THREADS), 0, s, sd, t0, n, dMult);
            a.ent_next = dEnt[cur]; a.act_next = dAct[cur]; a.act_off_next = dOff[cur]; a.large_next = dLarge[cur];
            hipLaunchKernelGGL(rf_root, dim3(Bc), dim3(THREADS), 0, s, dMult, a);
            HIPCHK(hipGetLastError());
            launches += 2;
            int cnts[2] = {0, 0};
            download<int>(cnts, a.counters, 2, s);
            ms[0] += now_ms() - t_mark;
            for (int level = 0; level <= MAX_DEPTH && cnts[0] > 0; ++level) {
                t_mark = now_ms();
                a.level = level; a.n_active = cnts[0]; a.n_large = cnts[1];
                a.ent = dEnt[cur]; a.act = dAct[cur]; a.act_off = dOff[cur]; a.large = dLarge[cur];
                a.ent_next = dEnt[cur ^ 1]; a.act_next = dAct[cur ^ 1]; a.act_off_next = dOff[cur ^ 1]; a.large_next = dLarge[cur ^ 1];
                if (a.n_large > 0) {
                    search_launch(rf_search<4, uint32_t>, once_large, device, a.n_large, lds_large, s, a);
                    ++launches;
                }
                if (a.n_large < a.n_active) {
                    search_launch(rf_search<1, uint16_t>, once_small, device, (a.n_active + 3) / 4, lds_small, s, a);
                    ++launches;
                }
                hipLaunchKernelGGL(rf_tree_scan, dim3(Bc), dim3(THREADS), 0, s, a);
                hipLaunchKernelGGL(rf_offsets, dim3(1), dim3(THREADS), 0, s, a);
                hipLaunchKernelGGL(rf_partition, dim3((a.n_active + 3) / 4), dim3(THREADS), 0, s, a);
                HIPCHK(hipGetLastError());
                launches += 3;
                download<int>(cnts, a.counters, 2, s);          // the one read per level: the next work list's lengths
                cur ^= 1;
                ms[2 + level] += now_ms() - t_mark;
            }
            t_mark = now_ms();
            hipLaunchKernelGGL(rf_predict, dim3((nte + THREADS - 1) / THREADS, Bc), dim3(THREADS), lds_predict, s, a.nodes, a.ncount, n,
                               dTbins, nte, C, dVotes);
            HIPCHK(hipGetLastError());
            ++launches;
            if (forest) {
                h_ncount.resize(Bc);
                h_nodes.resize((size_t)Bc * 2 * n);
                HIPCHK(hipMemcpyAsync(h_nodes.data(), a.nodes, h_nodes.size() * sizeof(int4), hipMemcpyDeviceToHost, s));
                download<int>(h_ncount.data(), a.ncount, Bc, s);
                for (int tb = 0; tb < Bc; ++tb) {
                    const size_t o = (size_t)(t0 + tb) * 2 * n;
                    f_nn[t0 + tb] = h_ncount[tb];
                    for (int q = 0; q < h_ncount[tb]; ++q) {
                        const int4 r = h_nodes[(size_t)tb * 2 * n + q];
                        f_feat[o + q] = r.x; f_thr[o + q] = r.y; f_left[o + q] = r.z; f_cls[o + q] = r.w;
                    }
                }
            } else {
                HIPCHK(hipStreamSynchronize(s));
            }
            ms[1] += now_ms() - t_mark;
        }
        std::vector<int> votes((size_t)nte * C);
        std::vector<double> lo(p), hi(p), prob((size_t)nte * C);
        HIPCHK(hipMemcpyAsync(lo.data(), dLo, (size_t)p * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hi.data(), dHi, (size_t)p * 8, hipMemcpyDeviceToHost, s));
        download<int>(votes.data(), dVotes, votes.size(), s);
        for (size_t q = 0; q < votes.size(); ++q) prob[q] = (double)votes[q] / (double)T;
        // the metrics stage of the kNN and logistic entries; it writes its outputs only when it succeeds, and is the last device work
        int st_metrics = -99, nte_ = nte, C_ = C;
        rcppml_gpu_classify_metrics_ex(prob.data(), test_labels, &nte_, &C_, out_predictions, out_confusion, out_precision, out_recall,
                                       out_f1, out_support, out_auc, &st_metrics);
        if (st_metrics != 0) throw std::runtime_error(std::string(rcppml_err()));
        launches += 3;
        std::copy(votes.begin(), votes.end(), out_votes);
        std::copy(prob.begin(), prob.end(), out_prob);
        if (forest) {
            std::copy(f_feat.begin(), f_feat.end(), out_feature);
            std::copy(f_thr.begin(), f_thr.end(), out_threshold);
            std::copy(f_left.begin(), f_left.end(), out_left);
            std::copy(f_cls.begin(), f_cls.end(), out_class);
            std::copy(f_nn.begin(), f_nn.end(), out_n_nodes);
            std::copy(lo.begin(), lo.end(), out_lo);
            std::copy(hi.begin(), hi.end(), out_hi);
        }
        if (out_ms) std::copy(ms.begin(), ms.end(), out_ms);
        if (out_launches) *out_launches = launches;
    });
}
