// ops_classify.hip -- classifier evaluation on the device (kernels: kernels_classify.hip.h) and its three build-defined entries:
// rcppml_gpu_classify_metrics_ex (confusion matrix, per-class precision / recall / F1 / support and one-vs-rest AUC from a
// probability matrix), rcppml_gpu_classify_knn_ex (exact fp32 kNN votes, then the metrics) and rcppml_gpu_classify_logistic_ex
// (C one-vs-rest binomial GLMs by IRLS with R's glm.fit arithmetic, then the metrics).  They are the device side of the
// reference's classify_embedding / classify_logistic (R/classifier_metrics.R:49-138, 219-291, 387-492).
//
// Every argument is checked before the device is touched, and outputs are written only after the last device call has returned,
// so a refused or failed call leaves every output buffer as it was.
#include "entry_common.hip.h"
#include "kernels_classify.hip.h"
#include "knn_launch.hip.h"

#include <climits>
#include <cmath>

namespace {
using namespace rcppml_plugin;
using namespace rcl;

struct Sizes { int ntr, nte, dim, C; };

void check_labels(const int* lab, int n, int C, const char* what) {
    for (int i = 0; i < n; ++i)
        if (lab[i] < 0 || lab[i] >= C) throw std::invalid_argument(std::string(what) + " holds a label outside [0, n_classes)");
}

void check_classes(int C) {
    if (C < 2 || C > 256) throw std::invalid_argument("n_classes must be in [2, 256]");
}

Sizes read_sizes(const double* train, const double* test, const int* train_labels, const int* test_labels, const int* n_train,
                 const int* n_test, const int* dim, const int* n_classes) {
    if (!n_train || !n_test || !dim || !n_classes) throw std::invalid_argument("null scalar argument");
    if (!train || !test || !train_labels || !test_labels) throw std::invalid_argument("null array");
    const Sizes z{*n_train, *n_test, *dim, *n_classes};
    if (z.ntr < 1 || z.nte < 1) throw std::invalid_argument("n_train and n_test must be >= 1");
    if (z.dim < 1 || z.dim > 128) throw std::invalid_argument("dim must be in [1, 128]");
    check_classes(z.C);
    check_labels(train_labels, z.ntr, z.C, "train_labels");
    check_labels(test_labels, z.nte, z.C, "test_labels");
    all_finite(train, (size_t)z.ntr * z.dim, "the training embedding");
    all_finite(test, (size_t)z.nte * z.dim, "the test embedding");
    return z;
}

struct MetricOuts {
    int* pred; int* conf; double* prec; double* rec; double* f1; int* support; double* auc;
    void check() const {
        if (!pred || !conf || !prec || !rec || !f1 || !support || !auc) throw std::invalid_argument("null output");
    }
};

struct Metrics {
    std::vector<int> pred, conf, support;
    std::vector<double> prec, rec, f1, auc;
    void write(const MetricOuts& o) const {
        std::copy(pred.begin(), pred.end(), o.pred);
        std::copy(conf.begin(), conf.end(), o.conf);
        std::copy(prec.begin(), prec.end(), o.prec);
        std::copy(rec.begin(), rec.end(), o.rec);
        std::copy(f1.begin(), f1.end(), o.f1);
        std::copy(support.begin(), support.end(), o.support);
        std::copy(auc.begin(), auc.end(), o.auc);
    }
};

size_t metric_bytes(int nte, int C) {
    return (size_t)nte * 8 + (size_t)C * C * 4 + (size_t)C * ((nte + THREADS - 1) / THREADS) * 8 + 4096;
}

// dProb nte x C, dTruth / dPred nte (device).  h_truth: the host copy of the test labels.
Metrics device_metrics(const double* dProb, const int* dTruth, const int* dPred, const int* h_truth, int nte, int C, hipStream_t s,
                       int& launches) {
    Metrics m;
    const int nb = (nte + THREADS - 1) / THREADS;
    DevBuf Cb, Ab;
    int* dConf = zeros<int>(Cb, (size_t)C * C, s);
    unsigned long long* dPairs = dalloc<unsigned long long>(Ab, (size_t)C * nb);
    hipLaunchKernelGGL(confusion_count, dim3(nb), dim3(THREADS), 0, s, dTruth, dPred, nte, C, dConf);
    hipLaunchKernelGGL(auc_pairs, dim3(nb, C), dim3(THREADS), 0, s, dProb, dTruth, nte, C, dPairs);
    HIPCHK(hipGetLastError());
    launches += 2;
    m.pred.resize(nte);
    m.conf.resize((size_t)C * C);
    std::vector<unsigned long long> pairs((size_t)C * nb);
    HIPCHK(hipMemcpyAsync(m.pred.data(), dPred, (size_t)nte * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(m.conf.data(), dConf, m.conf.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    download<unsigned long long>(pairs.data(), dPairs, pairs.size(), s);
    m.prec.assign(C, 0.0); m.rec.assign(C, 0.0); m.f1.assign(C, 0.0); m.auc.assign(C, 0.5); m.support.assign(C, 0);
    std::vector<long long> npos(C, 0);
    for (int i = 0; i < nte; ++i) npos[h_truth[i]]++;
    for (int c = 0; c < C; ++c) {
        long long row = 0, col = 0;
        for (int q = 0; q < C; ++q) { row += m.conf[(size_t)c * C + q]; col += m.conf[(size_t)q * C + c]; }
        const long long tp = m.conf[(size_t)c * C + c];
        const double prec = col > 0 ? (double)tp / (double)col : 0.0;
        const double rec = row > 0 ? (double)tp / (double)row : 0.0;
        m.prec[c] = prec;
        m.rec[c] = rec;
        m.f1[c] = (prec + rec) > 0 ? 2 * prec * rec / (prec + rec) : 0.0;
        m.support[c] = (int)row;
        const long long nneg = nte - npos[c];
        if (npos[c] > 0 && nneg > 0) {
            unsigned long long cnt = 0;
            for (int b = 0; b < nb; ++b) cnt += pairs[(size_t)c * nb + b];
            m.auc[c] = (double)cnt / ((double)npos[c] * (double)nneg);
        }
    }
    return m;
}

}  // namespace

extern "C" void rcppml_gpu_classify_metrics_ex(const double* prob, const int* test_labels, int* n_test, int* n_classes,
                                               int* out_predictions, int* out_confusion, double* out_precision, double* out_recall,
                                               double* out_f1, int* out_support, double* out_auc, int* out_status) {
    entry_guard(out_status, [&] {
        if (!n_test || !n_classes) throw std::invalid_argument("null scalar argument");
        if (!prob || !test_labels) throw std::invalid_argument("null array");
        const MetricOuts mo{out_predictions, out_confusion, out_precision, out_recall, out_f1, out_support, out_auc};
        mo.check();
        const int nte = *n_test, C = *n_classes;
        if (nte < 1) throw std::invalid_argument("n_test must be >= 1");
        check_classes(C);
        check_labels(test_labels, nte, C, "test_labels");
        all_finite(prob, (size_t)nte * C, "the probability matrix");
        device_ready((size_t)nte * C * 8 + metric_bytes(nte, C), "the classifier metrics");
        Stream st;
        DevBuf Pb, Tb, Rb;
        const double* dP = upload<double>(Pb, prob, (size_t)nte * C, st.s);
        const int* dT = upload<int>(Tb, test_labels, nte, st.s);
        int* dPred = dalloc<int>(Rb, nte);
        int launches = 1;
        hipLaunchKernelGGL(prob_argmax, dim3((nte + THREADS - 1) / THREADS), dim3(THREADS), 0, st.s, dP, nte, C, dPred);
        const Metrics m = device_metrics(dP, dT, dPred, test_labels, nte, C, st.s, launches);
        m.write(mo);
    });
}

extern "C" void rcppml_gpu_classify_knn_ex(const double* train, const double* test, const int* train_labels, const int* test_labels,
                                           int* n_train, int* n_test, int* dim, int* n_classes, int* k, int* distance,
                                           double* out_votes, int* out_predictions, int* out_confusion, double* out_precision,
                                           double* out_recall, double* out_f1, int* out_support, double* out_auc, int* out_launches,
                                           int* out_status) {
    entry_guard(out_status, [&] {
        const Sizes z = read_sizes(train, test, train_labels, test_labels, n_train, n_test, dim, n_classes);
        if (!k || !distance) throw std::invalid_argument("null scalar argument");
        const int K = *k;
        if (K < 1 || K > z.ntr) throw std::invalid_argument("k must be in [1, n_train]");
        if (*distance != 0 && *distance != 1) throw std::invalid_argument("distance must be 0 (euclidean) or 1 (cosine)");
        const MetricOuts mo{out_predictions, out_confusion, out_precision, out_recall, out_f1, out_support, out_auc};
        mo.check();
        if (!out_votes) throw std::invalid_argument("null output");
        const size_t etr = (size_t)z.ntr * z.dim, ete = (size_t)z.nte * z.dim, nk = (size_t)z.nte * K;
        // fp32 copies, the top-k lists and their per-split partials (at most 1 GiB, or 16 splits of small lists), votes, metrics
        device_ready((etr + ete) * 4 + nk * 8 + std::min<size_t>((size_t)1 << 30, nk * 8 * 4096) + nk * 8 + (size_t)z.nte * z.C * 8 +
                         (size_t)(z.ntr + z.nte) * 4 + metric_bytes(z.nte, z.C), "the kNN classifier");
        // fp32 rows; cosine: unit rows (a zero norm becomes 1), on which d^2 = 2 - 2 cos keeps the order
        auto rows32 = [&](const double* src, int n) {
            std::vector<float> out((size_t)n * z.dim);
            for (int i = 0; i < n; ++i) {
                double nrm = 1.0;
                if (*distance == 1) {
                    double s = 0.0;
                    for (int j = 0; j < z.dim; ++j) s += src[(size_t)i * z.dim + j] * src[(size_t)i * z.dim + j];
                    nrm = std::sqrt(s);
                    if (nrm == 0.0) nrm = 1.0;
                }
                for (int j = 0; j < z.dim; ++j) out[(size_t)i * z.dim + j] = (float)(src[(size_t)i * z.dim + j] / nrm);
            }
            return out;
        };
        const std::vector<float> htr = rows32(train, z.ntr), hte = rows32(test, z.nte);
        Stream st;
        DevBuf Ab, Bb, La, Lb, Ib, Db, Vb, Pb;
        const float* dTr = upload<float>(Ab, htr.data(), htr.size(), st.s);
        const float* dTe = upload<float>(Bb, hte.data(), hte.size(), st.s);
        const int* dLtr = upload<int>(La, train_labels, z.ntr, st.s);
        const int* dLte = upload<int>(Lb, test_labels, z.nte, st.s);
        int* dI = dalloc<int>(Ib, nk);
        float* dD = dalloc<float>(Db, nk);
        double* dV = dalloc<double>(Vb, (size_t)z.nte * z.C);
        int* dPred = dalloc<int>(Pb, z.nte);
        int launches = 0;
        knn_device(dTe, z.nte, dTr, z.ntr, z.dim, 0, nullptr, nullptr, K, K, dI, dD, st.s);
        launches += 2;
        hipLaunchKernelGGL(knn_vote, dim3(z.nte), dim3(64), (size_t)z.C * sizeof(int), st.s, dI, dLtr, z.nte, K, z.C, dV, dPred);
        HIPCHK(hipGetLastError());
        launches += 1;
        const Metrics m = device_metrics(dV, dLte, dPred, test_labels, z.nte, z.C, st.s, launches);
        std::vector<double> votes((size_t)z.nte * z.C);
        download<double>(votes.data(), dV, votes.size(), st.s);
        std::copy(votes.begin(), votes.end(), out_votes);
        m.write(mo);
        if (out_launches) *out_launches = launches;
    });
}

extern "C" void rcppml_gpu_classify_logistic_ex(const double* train, const double* test, const int* train_labels,
                                                const int* test_labels, int* n_train, int* n_test, int* dim, int* n_classes, int* maxit,
                                                double* epsilon, int* row_blocks, double* out_coef, int* out_aliased, int* out_iters,
                                                int* out_converged, double* out_deviance, double* out_prob, int* out_predictions,
                                                int* out_confusion, double* out_precision, double* out_recall, double* out_f1,
                                                int* out_support, double* out_auc, int* out_launches, int* out_status) {
    entry_guard(out_status, [&] {
        const Sizes z = read_sizes(train, test, train_labels, test_labels, n_train, n_test, dim, n_classes);
        if (!maxit || !epsilon) throw std::invalid_argument("null scalar argument");
        if (*maxit < 1) throw std::invalid_argument("maxit must be >= 1");
        if (!std::isfinite(*epsilon)) throw std::invalid_argument("epsilon must be finite");
        if (row_blocks && *row_blocks < 0) throw std::invalid_argument("row_blocks must be >= 0");
        const MetricOuts mo{out_predictions, out_confusion, out_precision, out_recall, out_f1, out_support, out_auc};
        mo.check();
        if (!out_coef || !out_aliased || !out_iters || !out_converged || !out_deviance || !out_prob)
            throw std::invalid_argument("null output");
        const int P = z.dim + 1, C = z.C;
        const int nchunk = (z.ntr + CHUNK - 1) / CHUNK;
        const size_t PP = (size_t)P * P, cp = (size_t)C * P;
        const size_t etr = (size_t)z.ntr * z.dim, ete = (size_t)z.nte * z.dim;
        device_ready((etr + ete) * 8 + (size_t)(z.ntr + z.nte) * 4 + (size_t)nchunk * C * (PP + P + 1) * 8 + C * PP * 8 + cp * 12 +
                         (size_t)C * 32 + (size_t)z.nte * C * 8 + metric_bytes(z.nte, C), "the logistic classifier");
        Stream st;
        DevBuf Xb, Tb, La, Lb, Bb, Gb, Rb, Db, Wb, Alb, Dnb, Itb, Cvb, Dvb, Dob, Nb, Prb, Pdb;
        IrlsArgs a{};
        a.X = upload<double>(Xb, train, etr, st.s);
        const double* dT = upload<double>(Tb, test, ete, st.s);
        a.y = upload<int>(La, train_labels, z.ntr, st.s);
        const int* dLte = upload<int>(Lb, test_labels, z.nte, st.s);
        a.n = z.ntr; a.p = z.dim; a.P = P; a.C = C; a.nchunk = nchunk;
        a.beta = zeros<double>(Bb, cp, st.s);
        a.Gp = dalloc<double>(Gb, (size_t)nchunk * C * PP);
        a.bp = dalloc<double>(Rb, (size_t)nchunk * cp);
        a.dp = dalloc<double>(Db, (size_t)nchunk * C);
        a.A = dalloc<double>(Wb, C * PP);
        a.aliased = zeros<int>(Alb, cp, st.s);
        a.done = zeros<int>(Dnb, C, st.s);
        a.iters = zeros<int>(Itb, C, st.s);
        a.converged = zeros<int>(Cvb, C, st.s);
        a.deviance = zeros<double>(Dvb, C, st.s);
        a.devold = zeros<double>(Dob, C, st.s);
        a.ndone = zeros<int>(Nb, 1, st.s);
        a.maxit = *maxit;
        a.epsilon = *epsilon;
        // one workgroup per 128-row chunk; row_blocks > 0 (a test switch) takes that many workgroups, each looping over chunks
        const int blocks = (row_blocks && *row_blocks > 0) ? std::min(*row_blocks, nchunk) : nchunk;
        const size_t lds = irls_pass_lds_doubles(P) * sizeof(double);
        int launches = 0, ndone = 0;
        // launch L: pass (deviance of solve L - 1, Gram of solve L), then the convergence decision and solve L.  The host reads one
        // word per iteration: the number of classes done.
        for (int L = 1; L <= a.maxit + 1 && ndone < C; ++L) {
            hipLaunchKernelGGL(irls_pass, dim3(blocks), dim3(THREADS), lds, st.s, a, L == 1 ? 1 : 0);
            hipLaunchKernelGGL(irls_solve, dim3(C), dim3(THREADS), 0, st.s, a, L);
            HIPCHK(hipGetLastError());
            launches += 2;
            if (L > 1) download<int>(&ndone, a.ndone, 1, st.s);
        }
        double* dProb = dalloc<double>(Prb, (size_t)z.nte * C);
        int* dPred = dalloc<int>(Pdb, z.nte);
        hipLaunchKernelGGL(logit_predict, dim3((z.nte + THREADS - 1) / THREADS), dim3(THREADS), 0, st.s, dT, z.nte, z.dim, a.beta, C,
                           dProb, dPred);
        HIPCHK(hipGetLastError());
        launches += 1;
        const Metrics m = device_metrics(dProb, dLte, dPred, test_labels, z.nte, C, st.s, launches);
        std::vector<double> coef(cp), dev(C), prob((size_t)z.nte * C);
        std::vector<int> al(cp), it(C), cv(C);
        HIPCHK(hipMemcpyAsync(coef.data(), a.beta, cp * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(dev.data(), a.deviance, (size_t)C * 8, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(al.data(), a.aliased, cp * 4, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(it.data(), a.iters, (size_t)C * 4, hipMemcpyDeviceToHost, st.s));
        HIPCHK(hipMemcpyAsync(cv.data(), a.converged, (size_t)C * 4, hipMemcpyDeviceToHost, st.s));
        download<double>(prob.data(), dProb, prob.size(), st.s);
        std::copy(coef.begin(), coef.end(), out_coef);
        std::copy(al.begin(), al.end(), out_aliased);
        std::copy(it.begin(), it.end(), out_iters);
        std::copy(cv.begin(), cv.end(), out_converged);
        std::copy(dev.begin(), dev.end(), out_deviance);
        std::copy(prob.begin(), prob.end(), out_prob);
        m.write(mo);
        if (out_launches) *out_launches = launches;
    });
}
