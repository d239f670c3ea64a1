// ops_assess.hip -- embedding assessment on the device (kernels: kernels_assess.hip.h) and its entries: the reference plugin's
// rcppml_gpu_assess (src/gpu_bridge_assess.cu:358-753, 26 pointers), the build-defined rcppml_gpu_assess_ex (per-item results),
// rcppml_gpu_knn_float (the exact kNN on its own) and rcppml_gpu_assess_plan (the host-side random plan, no device work).
//
// The random plan is the reference's: std::mt19937 and std::shuffle from (unsigned)seed + offset.  ARI, NMI, the kNN votes, F1 and the
// batch entropy are computed on the host from device results.  The one deliberate deviation: the k-means centroid sums are fp64 in a
// fixed order, rounded to fp32 and divided in fp32, where the reference adds fp32 atomics (no fixed answer).
//
// Both kNN passes are one masked self-kNN over all n points: the classification folds exclude the query's own fold (k set per fold;
// the training order of the reference is ascending index, so its train-list ties are index ties), the batch pass excludes the query
// itself.  The reference takes k + 1 neighbours with self and drops self; that is the top k of the candidates other than self, also
// when duplicates push self out of its list.
#include "entry_common.hip.h"
#include "kernels_assess.hip.h"
#include "knn_launch.hip.h"

#include <climits>
#include <cmath>
#include <limits>
#include <random>

namespace {
using namespace rcppml_plugin;
using namespace ras;

// compile-time width of the register paths (0: the general path)
int bucket(int dim) { return dim <= 8 ? 8 : dim <= 16 ? 16 : dim <= 32 ? 32 : dim <= 64 ? 64 : 0; }

// ------------------------------------------------------------------------------------------------------------ exact kNN
constexpr size_t kKnnLds = 40 << 10;          // LDS budget of one kNN workgroup (queries + lists)
constexpr int kKnnTargetGroups = 4096;        // workgroups the candidate splits aim for (256 CUs x 16 waves)
constexpr size_t kKnnPartialBytes = size_t(1) << 30;

template <int DB> void launch_partial(const KnnArgs& a, int nsplit, size_t lds, hipStream_t s) {
    dim3 grid((a.nq + a.qpw - 1) / a.qpw, nsplit);
    hipLaunchKernelGGL(knn_partial<DB>, grid, dim3(WAVE), lds, s, a);
}

}  // namespace

// dQ nq x dim, dC nc x dim (device).  out: nq x kmax.  gk (device, mode 2) may be null.  Declared in knn_launch.hip.h: the
// classifier entries (ops_classify.hip) run the same top-k.
void rcppml_plugin::knn_device(const float* dQ, int nq, const float* dC, int nc, int dim, int mode, const int* dgroup, const int* dgk, int k, int kmax,
                int* d_oi, float* d_od, hipStream_t s) {
    KnnArgs a{};
    a.Q = dQ; a.C = dC; a.nq = nq; a.nc = nc; a.dim = dim; a.mode = mode; a.group = dgroup; a.gk = dgk; a.k = k; a.kmax = kmax;
    const int db = bucket(dim);
    a.qpw = 32;
    auto need = [&](int q, bool lists) { return (size_t)q * db * 4 + (lists ? (size_t)q * kmax * 8 : 0); };
    while (a.qpw > 8 && need(a.qpw, true) > kKnnLds) a.qpw /= 2;
    a.lists_lds = need(a.qpw, true) <= kKnnLds;
    if (!a.lists_lds) a.qpw = 32;
    const size_t lds = need(a.qpw, a.lists_lds);
    const long groups = (nq + a.qpw - 1) / a.qpw;
    long nsplit = std::max<long>(1, (kKnnTargetGroups + groups - 1) / groups);
    nsplit = std::min<long>(nsplit, std::max<long>(1, nc / 256));
    const size_t per_split = (size_t)nq * kmax * (sizeof(float) + sizeof(int));
    nsplit = std::max<long>(1, std::min<long>(nsplit, (long)(kKnnPartialBytes / std::max<size_t>(per_split, 1))));
    nsplit = std::min<long>(nsplit, 65535);
    long len = (nc + nsplit - 1) / nsplit;
    len = (len + WAVE - 1) / WAVE * WAVE;
    nsplit = (nc + len - 1) / len;
    a.split_len = (int)len;
    DevBuf pd, pi;
    a.pd = dalloc<float>(pd, (size_t)nsplit * nq * kmax);
    a.pi = dalloc<int>(pi, (size_t)nsplit * nq * kmax);
    switch (db) {
        case 8: launch_partial<8>(a, (int)nsplit, lds, s); break;
        case 16: launch_partial<16>(a, (int)nsplit, lds, s); break;
        case 32: launch_partial<32>(a, (int)nsplit, lds, s); break;
        case 64: launch_partial<64>(a, (int)nsplit, lds, s); break;
        default: launch_partial<0>(a, (int)nsplit, lds, s); break;
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(knn_merge, dim3((nq + 255) / 256), dim3(256), 0, s, a, (int)nsplit, d_oi, d_od);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));   // the partial buffers are freed on return
}

namespace {

// ------------------------------------------------------------------------------------------------------------ random plan
std::vector<int> kmeans_init(int n, int K, int nstart, unsigned seed) {
    std::vector<int> out((size_t)std::max(nstart, 0) * K);
    std::vector<int> idx(n);
    for (int r = 0; r < nstart; ++r) {
        std::mt19937 rng(seed + (unsigned)r);
        std::iota(idx.begin(), idx.end(), 0);
        std::shuffle(idx.begin(), idx.end(), rng);
        for (int c = 0; c < K; ++c) out[(size_t)r * K + c] = idx[c % n];
    }
    return out;
}

// per-class counts min(spc, size) and the samples of the classes in class order (max(count, 0) each)
void sil_plan(const int* labels, int n, int nc, int spc, unsigned seed, std::vector<int>& samples, std::vector<int>& counts) {
    std::mt19937 rng(seed + 100u);
    std::vector<std::vector<int>> cls(nc);
    for (int i = 0; i < n; ++i)
        if (labels[i] >= 0 && labels[i] < nc) cls[labels[i]].push_back(i);
    samples.clear();
    counts.assign(nc, 0);
    for (int c = 0; c < nc; ++c) {
        auto& idx = cls[c];
        counts[c] = std::min(spc, (int)idx.size());
        std::shuffle(idx.begin(), idx.end(), rng);
        for (int s = 0; s < counts[c]; ++s) samples.push_back(idx[s]);
    }
}

std::vector<int> fold_plan(const int* labels, int n, int nc, int folds, unsigned seed) {
    std::mt19937 rng(seed + 200u);
    std::vector<int> fold(n, 0), idx;
    for (int c = 0; c < nc; ++c) {
        idx.clear();
        for (int i = 0; i < n; ++i)
            if (labels[i] == c) idx.push_back(i);
        std::shuffle(idx.begin(), idx.end(), rng);
        for (int p = 0; p < (int)idx.size(); ++p) fold[idx[p]] = p % folds;
    }
    return fold;
}

// ------------------------------------------------------------------------------------------------------------ ARI / NMI
// Contingency table of truth (rows) x assignment (columns), each sized by its largest label + 1.
struct Table {
    int na = 0, nb = 0;
    std::vector<int> ct;
    Table(const int* a, const int* b, int n) {
        int ma = 0, mb = 0;
        for (int i = 0; i < n; ++i) { ma = std::max(ma, a[i]); mb = std::max(mb, b[i]); }
        na = ma + 1; nb = mb + 1;
        ct.assign((size_t)na * nb, 0);
        for (int i = 0; i < n; ++i) ct[(size_t)a[i] * nb + b[i]]++;
    }
};

double ari(const int* a, const int* b, int n) {
    Table t(a, b, n);
    std::vector<int> rs(t.na, 0), cs(t.nb, 0);
    for (int i = 0; i < t.na; ++i)
        for (int j = 0; j < t.nb; ++j) { rs[i] += t.ct[(size_t)i * t.nb + j]; cs[j] += t.ct[(size_t)i * t.nb + j]; }
    auto c2 = [](long long x) { return x * (x - 1) / 2.0; };
    double sij = 0, si = 0, sj = 0;
    for (int v : t.ct) sij += c2(v);
    for (int v : rs) si += c2(v);
    for (int v : cs) sj += c2(v);
    const double expected = si * sj / c2(n);
    const double den = 0.5 * (si + sj) - expected;
    return den == 0.0 ? 0.0 : (sij - expected) / den;
}

double nmi(const int* a, const int* b, int n) {
    Table t(a, b, n);
    std::vector<double> pi(t.na, 0.0), pj(t.nb, 0.0);
    for (int i = 0; i < t.na; ++i)
        for (int j = 0; j < t.nb; ++j) {
            const double v = (double)t.ct[(size_t)i * t.nb + j] / n;
            pi[i] += v;
            pj[j] += v;
        }
    double ha = 0, hb = 0, mi = 0;
    for (double p : pi) if (p > 0) ha -= p * std::log(p);
    for (double p : pj) if (p > 0) hb -= p * std::log(p);
    for (int i = 0; i < t.na; ++i)
        for (int j = 0; j < t.nb; ++j) {
            const double p = (double)t.ct[(size_t)i * t.nb + j] / n;
            if (p > 0 && pi[i] > 0 && pj[j] > 0) mi += p * std::log(p / (pi[i] * pj[j]));
        }
    const double den = std::sqrt(ha * hb);
    return den == 0.0 ? 0.0 : mi / den;
}

// ------------------------------------------------------------------------------------------------------------ assessment
struct In {
    const double* emb; int n, dim;
    const int* labels; int nc;
    const int* batch; int nbatch;
    bool clust, sil, clf, bat;
    int nstart, maxiter, spc, knn_k, folds, batch_k;
    unsigned seed;
};

struct Out {
    double ari = 0, nmi = 0, sil = 0, acc = 0, f1 = 0, bsil = 0, bent = 0;
    std::vector<int> assign, fold_ids;
    std::vector<double> r_ari, r_nmi, fold_acc, fold_f1, bent_pt, bsil_pt;
    std::vector<float> sil_pt;
};

In read_in(const double* emb, int* n, int* dim, const int* labels, int* nc, const int* batch, int* nbatch, int* dc, int* ds, int* dk,
           int* db, int* nstart, int* maxiter, int* spc, int* knn_k, int* folds, int* batch_k, int* seed) {
    if (!n || !dim || !nc || !nbatch || !dc || !ds || !dk || !db || !nstart || !maxiter || !spc || !knn_k || !folds || !batch_k || !seed)
        throw std::invalid_argument("null scalar argument");
    In in{emb, *n, *dim, labels, *nc, batch, *nbatch, *dc != 0, *ds != 0, *dk != 0, *db != 0 && *nbatch > 1,
          *nstart, *maxiter, *spc, *knn_k, *folds, *batch_k, (unsigned)*seed};
    if (in.n < 1) throw std::invalid_argument("n must be >= 1");
    if (in.dim < 1) throw std::invalid_argument("dim must be >= 1");
    if ((size_t)in.n * in.dim > (size_t)INT_MAX * 4) throw std::invalid_argument("n * dim is too large");
    if (!emb) throw std::invalid_argument("null embedding");
    if (in.clust && in.maxiter < 1) throw std::invalid_argument("kmeans_maxiter must be >= 1 for clustering");
    if (in.clust && in.nc < 1) throw std::invalid_argument("n_classes must be >= 1 for clustering");
    if (in.clf && in.knn_k < 1) throw std::invalid_argument("knn_k must be >= 1 for classification");
    if (in.clf && in.folds < 1) throw std::invalid_argument("knn_folds must be >= 1 for classification");
    if (in.bat && in.batch_k < 1) throw std::invalid_argument("batch_knn_k must be >= 1 for batch mixing");
    if (in.clust || in.sil || in.clf) {
        if (!labels) throw std::invalid_argument("null labels");
        for (int i = 0; i < in.n; ++i)
            if (labels[i] < 0 || labels[i] >= in.nc) throw std::invalid_argument("a label lies outside [0, n_classes)");
    }
    if (in.bat) {
        if (!batch) throw std::invalid_argument("null batch labels");
        for (int i = 0; i < in.n; ++i)
            if (batch[i] < 0 || batch[i] >= in.nbatch) throw std::invalid_argument("a batch label lies outside [0, n_batch)");
    }
    return in;
}

constexpr int kKmBlockPoints = 256;                 // points per k-means partial-sum block
constexpr int kKmRestartsPerLaunch = 16;
constexpr size_t kKmPartialBytes = size_t(256) << 20;

template <int DB> void km_assign_launch(const float* dX, int n, int dim, const float* dC, int K, int cs, int* dA, int R, hipStream_t s) {
    hipLaunchKernelGGL(km_assign<DB>, dim3((n + 255) / 256, R), dim3(256), 0, s, dX, n, dim, dC, K, cs, dA);
}

struct Engine {
    const In& in;
    Stream st;
    DevBuf X;
    const float* dX = nullptr;
    std::vector<float> h;

    explicit Engine(const In& i) : in(i) {
        h.resize((size_t)in.n * in.dim);
        for (size_t e = 0; e < h.size(); ++e) h[e] = (float)in.emb[e];
        dX = upload<float>(X, h.data(), h.size(), st.s);
    }

    // R restarts starting at r0; assignments of those restarts -> asg (R x n)
    void kmeans(int r0, int R, std::vector<int>& asg) {
        const int n = in.n, dim = in.dim, K = in.nc, db = bucket(dim), cs = db ? db : dim;
        std::vector<float> c0((size_t)R * K * cs, 0.f);
        for (int r = 0; r < R; ++r) {
            const std::vector<int> idx = kmeans_init(n, K, 1, in.seed + (unsigned)(r0 + r));
            for (int c = 0; c < K; ++c)
                for (int j = 0; j < dim; ++j) c0[((size_t)r * K + c) * cs + j] = h[(size_t)idx[c] * dim + j];
        }
        DevBuf Cb, Ab, Pb, Nb;
        float* dC = upload<float>(Cb, c0.data(), c0.size(), st.s);
        int* dA = dalloc<int>(Ab, (size_t)R * n);
        int bp = kKmBlockPoints;
        int nb = (n + bp - 1) / bp;
        const size_t per_block = (size_t)R * K * dim * sizeof(double);
        if ((size_t)nb * per_block > kKmPartialBytes) {
            nb = (int)std::max<size_t>(1, kKmPartialBytes / per_block);
            bp = (n + nb - 1) / nb;
            nb = (n + bp - 1) / bp;
        }
        double* dP = dalloc<double>(Pb, (size_t)R * nb * K * dim);
        int* dN = dalloc<int>(Nb, (size_t)R * nb * K);
        const size_t acc_lds = (size_t)K * dim * sizeof(double) + (size_t)K * sizeof(int);
        const bool lds_acc = acc_lds <= (48 << 10);
        const size_t nfin = (size_t)R * K * dim;
        for (int it = 0; it < in.maxiter; ++it) {
            switch (db) {
                case 8: km_assign_launch<8>(dX, n, dim, dC, K, cs, dA, R, st.s); break;
                case 16: km_assign_launch<16>(dX, n, dim, dC, K, cs, dA, R, st.s); break;
                case 32: km_assign_launch<32>(dX, n, dim, dC, K, cs, dA, R, st.s); break;
                case 64: km_assign_launch<64>(dX, n, dim, dC, K, cs, dA, R, st.s); break;
                default: km_assign_launch<0>(dX, n, dim, dC, K, cs, dA, R, st.s); break;
            }
            if (lds_acc) hipLaunchKernelGGL(km_accum<true>, dim3(nb, R), dim3(WAVE), acc_lds, st.s, dX, n, dim, dA, K, bp, dP, dN);
            else hipLaunchKernelGGL(km_accum<false>, dim3(nb, R), dim3(WAVE), 0, st.s, dX, n, dim, dA, K, bp, dP, dN);
            hipLaunchKernelGGL(km_finalize, dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, st.s, dP, dN, R, nb, K, dim, cs, dC);
        }
        HIPCHK(hipGetLastError());
        asg.resize((size_t)R * n);
        download<int>(asg.data(), dA, asg.size(), st.s);
    }

    void clustering(Out& o) {
        const int n = in.n;
        o.ari = -1.0; o.nmi = -1.0;
        o.r_ari.assign(std::max(in.nstart, 0), 0.0);
        o.r_nmi.assign(std::max(in.nstart, 0), 0.0);
        std::vector<int> asg;
        for (int r0 = 0; r0 < in.nstart; r0 += kKmRestartsPerLaunch) {
            const int R = std::min(kKmRestartsPerLaunch, in.nstart - r0);
            kmeans(r0, R, asg);
            for (int r = 0; r < R; ++r) {
                const int* a = asg.data() + (size_t)r * n;
                const double ar = ari(in.labels, a, n), nm = nmi(in.labels, a, n);
                o.r_ari[r0 + r] = ar;
                o.r_nmi[r0 + r] = nm;
                if (ar > o.ari) { o.ari = ar; o.nmi = nm; o.assign.assign(a, a + n); }
            }
        }
    }

    void silhouette(Out& o) {
        const int n = in.n, dim = in.dim, nc = in.nc;
        std::vector<int> samples, counts;
        sil_plan(in.labels, n, nc, in.spc, in.seed, samples, counts);
        o.sil_pt.assign(n, 0.f);
        if (in.spc < 0) {
            // every class count is spc < 0: the reference's mean is 0 / (float)count = -0 for every class, so a = b = -0 (s = 0), or
            // with one class b stays 1e30 and s = (1e30 - a) / 1e30 = 1
            std::fill(o.sil_pt.begin(), o.sil_pt.end(), nc >= 2 ? 0.f : 1.f);
        } else {
            const int db = bucket(dim), cs = db ? db : dim;
            const int stot = (int)samples.size();
            std::vector<float> S((size_t)std::max(stot, 1) * cs, 0.f);
            for (int s = 0; s < stot; ++s)
                for (int j = 0; j < dim; ++j) S[(size_t)s * cs + j] = h[(size_t)samples[s] * dim + j];
            std::vector<int> rcls, roff, rcnt;
            int off = 0;
            for (int c = 0; c < nc; ++c) {
                if (counts[c] > 0) { rcls.push_back(c); roff.push_back(off); rcnt.push_back(counts[c]); }
                off += counts[c];
            }
            const int nr = (int)rcls.size();
            DevBuf Sb, Lb, Cb, Ob, Nb, Rb;
            const float* dS = upload<float>(Sb, S.data(), S.size(), st.s);
            const int* dL = upload<int>(Lb, in.labels, n, st.s);
            const int* dc = upload<int>(Cb, rcls.data(), nr, st.s);
            const int* dof = upload<int>(Ob, roff.data(), nr, st.s);
            const int* dn = upload<int>(Nb, rcnt.data(), nr, st.s);
            float* dR = dalloc<float>(Rb, n);
            const dim3 g((n + 255) / 256), b(256);
            switch (db) {
                case 8: hipLaunchKernelGGL(sil_kernel<8>, g, b, 0, st.s, dX, n, dim, dL, dS, stot, cs, dc, dof, dn, nr, dR); break;
                case 16: hipLaunchKernelGGL(sil_kernel<16>, g, b, 0, st.s, dX, n, dim, dL, dS, stot, cs, dc, dof, dn, nr, dR); break;
                case 32: hipLaunchKernelGGL(sil_kernel<32>, g, b, 0, st.s, dX, n, dim, dL, dS, stot, cs, dc, dof, dn, nr, dR); break;
                case 64: hipLaunchKernelGGL(sil_kernel<64>, g, b, 0, st.s, dX, n, dim, dL, dS, stot, cs, dc, dof, dn, nr, dR); break;
                default: hipLaunchKernelGGL(sil_kernel<0>, g, b, 0, st.s, dX, n, dim, dL, dS, stot, cs, dc, dof, dn, nr, dR); break;
            }
            HIPCHK(hipGetLastError());
            download<float>(o.sil_pt.data(), dR, n, st.s);
        }
        double sum = 0;
        for (int i = 0; i < n; ++i) sum += o.sil_pt[i];
        o.sil = sum / n;
    }

    void classify(Out& o) {
        const int n = in.n, nc = in.nc, F = in.folds;
        o.fold_ids = fold_plan(in.labels, n, nc, F, in.seed);
        std::vector<int> ntest(F, 0), kf(F, 0);
        for (int i = 0; i < n; ++i) ntest[o.fold_ids[i]]++;
        int kmax = 0;
        for (int f = 0; f < F; ++f) {
            const int ntr = n - ntest[f];
            kf[f] = (ntr > 0 && ntest[f] > 0) ? std::min(in.knn_k, ntr) : 0;
            kmax = std::max(kmax, kf[f]);
        }
        std::vector<int> nn((size_t)n * std::max(kmax, 1), -1);
        if (kmax > 0) {
            DevBuf Gb, Kb, Ib, Db;
            const int* dg = upload<int>(Gb, o.fold_ids.data(), n, st.s);
            const int* dk = upload<int>(Kb, kf.data(), F, st.s);
            int* di = dalloc<int>(Ib, (size_t)n * kmax);
            float* dd = dalloc<float>(Db, (size_t)n * kmax);
            knn_device(dX, n, dX, n, in.dim, 2, dg, dk, kmax, kmax, di, dd, st.s);
            download<int>(nn.data(), di, (size_t)n * kmax, st.s);
        }
        o.fold_acc.assign(F, std::numeric_limits<double>::quiet_NaN());
        o.fold_f1.assign(F, std::numeric_limits<double>::quiet_NaN());
        double tacc = 0, tf1 = 0;
        int valid = 0;
        std::vector<int> votes(nc), tp(nc), fp(nc), fn(nc);
        for (int f = 0; f < F; ++f) {
            if (!(n - ntest[f] > 0 && ntest[f] > 0)) continue;
            std::fill(tp.begin(), tp.end(), 0); std::fill(fp.begin(), fp.end(), 0); std::fill(fn.begin(), fn.end(), 0);
            int correct = 0;
            for (int i = 0; i < n; ++i) {
                if (o.fold_ids[i] != f) continue;
                std::fill(votes.begin(), votes.end(), 0);
                for (int e = 0; e < kf[f]; ++e) {
                    const int j = nn[(size_t)i * kmax + e];
                    if (j >= 0) votes[in.labels[j]]++;
                }
                const int pred = (int)(std::max_element(votes.begin(), votes.end()) - votes.begin());
                const int truth = in.labels[i];
                if (pred == truth) { correct++; tp[truth]++; }
                else { fp[pred]++; fn[truth]++; }
            }
            const double acc = (double)correct / ntest[f];
            double f1s = 0;
            for (int c = 0; c < nc; ++c) {
                const double prec = (tp[c] + fp[c]) > 0 ? (double)tp[c] / (tp[c] + fp[c]) : 0;
                const double rec = (tp[c] + fn[c]) > 0 ? (double)tp[c] / (tp[c] + fn[c]) : 0;
                f1s += (prec + rec) > 0 ? 2.0 * prec * rec / (prec + rec) : 0;
            }
            const double f1 = f1s / std::max(nc, 1);
            o.fold_acc[f] = acc;
            o.fold_f1[f] = f1;
            tacc += acc;
            tf1 += f1;
            valid++;
        }
        o.acc = valid > 0 ? tacc / valid : 0;
        o.f1 = valid > 0 ? tf1 / valid : 0;
    }

    void batch(Out& o) {
        const int n = in.n, B = in.nbatch;
        const int k = std::min(in.batch_k, n - 1);
        std::vector<int> nn((size_t)n * std::max(k, 1), -1);
        std::vector<float> nd((size_t)n * std::max(k, 1), kBig);
        if (k > 0) {
            DevBuf Ib, Db;
            int* di = dalloc<int>(Ib, (size_t)n * k);
            float* dd = dalloc<float>(Db, (size_t)n * k);
            knn_device(dX, n, dX, n, in.dim, 1, nullptr, nullptr, k, k, di, dd, st.s);
            download<int>(nn.data(), di, (size_t)n * k, st.s);
            download<float>(nd.data(), dd, (size_t)n * k, st.s);
        }
        const double hmax = std::log((double)B);
        o.bent_pt.assign(n, 0.0);
        o.bsil_pt.assign(n, 0.0);
        double esum = 0, ssum = 0;
        std::vector<int> votes(B);
        for (int i = 0; i < n; ++i) {
            std::fill(votes.begin(), votes.end(), 0);
            double as = 0, bs = 0;
            int ac = 0, bc = 0, cnt = 0;
            const int mine = in.batch[i];
            for (int e = 0; e < k; ++e) {
                const int j = nn[(size_t)i * k + e];
                if (j < 0) continue;
                votes[in.batch[j]]++;
                const float d = std::sqrt(std::max(nd[(size_t)i * k + e], 0.0f));
                if (in.batch[j] == mine) { as += d; ac++; }
                else { bs += d; bc++; }
                cnt++;
            }
            double ent = 0;
            for (int b = 0; b < B; ++b)
                if (votes[b] > 0) {
                    const double p = (double)votes[b] / cnt;
                    ent -= p * std::log(p);
                }
            const double e = hmax > 0 ? ent / hmax : 0;
            const double ai = ac > 0 ? as / ac : 0;
            const double bi = bc > 0 ? bs / bc : ai;
            const double den = std::max(ai, bi);
            const double s = den > 0 ? (bi - ai) / den : 0;
            o.bent_pt[i] = e;
            o.bsil_pt[i] = s;
            esum += e;
            ssum += s;
        }
        o.bent = esum / n;
        o.bsil = ssum / n;
    }

    void run(Out& o) {
        if (in.clust) clustering(o);
        if (in.sil) silhouette(o);
        if (in.clf) classify(o);
        if (in.bat) batch(o);
    }
};

#define ASSESS_PARAMS                                                                                                              \
    const double *embedding, int *n, int *dim, const int *labels, int *n_classes, const int *batch_labels, int *n_batch,            \
        int *do_clustering, int *do_silhouette, int *do_classify, int *do_batch, int *kmeans_nstart, int *kmeans_maxiter,            \
        int *sil_samples_per_class, int *knn_k, int *knn_folds, int *batch_knn_k, int *seed, double *out_ari, double *out_nmi,      \
        double *out_silhouette, double *out_knn_accuracy, double *out_knn_f1, double *out_batch_sil, double *out_batch_entropy
#define ASSESS_READ                                                                                                                \
    read_in(embedding, n, dim, labels, n_classes, batch_labels, n_batch, do_clustering, do_silhouette, do_classify, do_batch,       \
            kmeans_nstart, kmeans_maxiter, sil_samples_per_class, knn_k, knn_folds, batch_knn_k, seed)

void write_scalars(const In& in, const Out& o, double* out_ari, double* out_nmi, double* out_silhouette, double* out_knn_accuracy,
                   double* out_knn_f1, double* out_batch_sil, double* out_batch_entropy) {
    if (in.clust) { *out_ari = o.ari; *out_nmi = o.nmi; }
    if (in.sil) *out_silhouette = o.sil;
    if (in.clf) { *out_knn_accuracy = o.acc; *out_knn_f1 = o.f1; }
    if (in.bat) { *out_batch_sil = o.bsil; *out_batch_entropy = o.bent; }
}

void check_scalar_outputs(const In& in, double* out_ari, double* out_nmi, double* out_silhouette, double* out_knn_accuracy,
                          double* out_knn_f1, double* out_batch_sil, double* out_batch_entropy) {
    if ((in.clust && (!out_ari || !out_nmi)) || (in.sil && !out_silhouette) || (in.clf && (!out_knn_accuracy || !out_knn_f1)) ||
        (in.bat && (!out_batch_sil || !out_batch_entropy)))
        throw std::invalid_argument("null output");
}

// the assessment on the device RCPPML_GPU_DEVICE names (selected before the engine's stream is made)
Out run_engine(const In& in) {
    HIPCHK(hipSetDevice(env_device()));
    Out o;
    Engine E(in);
    E.run(o);
    return o;
}

void need(bool used, const int* cap, long count, const char* what) {
    if (!used) return;
    if (!cap || *cap < count) throw std::invalid_argument(std::string(what) + " is too small");
}

}  // namespace

extern "C" void rcppml_gpu_assess(ASSESS_PARAMS, int* out_status) {
    entry_guard(out_status, [&] {
        const In in = ASSESS_READ;
        check_scalar_outputs(in, out_ari, out_nmi, out_silhouette, out_knn_accuracy, out_knn_f1, out_batch_sil, out_batch_entropy);
        const Out o = run_engine(in);
        write_scalars(in, o, out_ari, out_nmi, out_silhouette, out_knn_accuracy, out_knn_f1, out_batch_sil, out_batch_entropy);
    });
}

extern "C" void rcppml_gpu_assess_ex(ASSESS_PARAMS, int* out_assignments, double* out_restart_ari, double* out_restart_nmi,
                                     float* out_sil_point, int* out_fold_ids, double* out_fold_accuracy, double* out_fold_f1,
                                     double* out_batch_entropy_point, double* out_batch_sil_point, int* point_capacity,
                                     int* restart_capacity, int* fold_capacity, int* out_status) {
    entry_guard(out_status, [&] {
        const In in = ASSESS_READ;
        check_scalar_outputs(in, out_ari, out_nmi, out_silhouette, out_knn_accuracy, out_knn_f1, out_batch_sil, out_batch_entropy);
        need(in.clust && out_assignments, point_capacity, in.n, "point_capacity");
        need(in.sil && out_sil_point, point_capacity, in.n, "point_capacity");
        need(in.clf && out_fold_ids, point_capacity, in.n, "point_capacity");
        need(in.bat && (out_batch_entropy_point || out_batch_sil_point), point_capacity, in.n, "point_capacity");
        need(in.clust && (out_restart_ari || out_restart_nmi), restart_capacity, in.nstart, "restart_capacity");
        need(in.clf && (out_fold_accuracy || out_fold_f1), fold_capacity, in.folds, "fold_capacity");
        const Out o = run_engine(in);
        write_scalars(in, o, out_ari, out_nmi, out_silhouette, out_knn_accuracy, out_knn_f1, out_batch_sil, out_batch_entropy);
        if (in.clust) {
            if (out_assignments && !o.assign.empty()) std::copy(o.assign.begin(), o.assign.end(), out_assignments);
            if (out_restart_ari) std::copy(o.r_ari.begin(), o.r_ari.end(), out_restart_ari);
            if (out_restart_nmi) std::copy(o.r_nmi.begin(), o.r_nmi.end(), out_restart_nmi);
        }
        if (in.sil && out_sil_point) std::copy(o.sil_pt.begin(), o.sil_pt.end(), out_sil_point);
        if (in.clf) {
            if (out_fold_ids) std::copy(o.fold_ids.begin(), o.fold_ids.end(), out_fold_ids);
            if (out_fold_accuracy) std::copy(o.fold_acc.begin(), o.fold_acc.end(), out_fold_accuracy);
            if (out_fold_f1) std::copy(o.fold_f1.begin(), o.fold_f1.end(), out_fold_f1);
        }
        if (in.bat) {
            if (out_batch_entropy_point) std::copy(o.bent_pt.begin(), o.bent_pt.end(), out_batch_entropy_point);
            if (out_batch_sil_point) std::copy(o.bsil_pt.begin(), o.bsil_pt.end(), out_batch_sil_point);
        }
    });
}

extern "C" void rcppml_gpu_knn_float(const float* query, int* n_query, const float* train, int* n_train, int* dim, int* k,
                                     int* mask_mode, const int* group, const int* group_k, int* n_groups, int* out_idx,
                                     float* out_dist, int* out_capacity, int* out_status) {
    entry_guard(out_status, [&] {
        if (!n_query || !dim || !k || !mask_mode || !out_capacity) throw std::invalid_argument("null scalar argument");
        const int nq = *n_query, d = *dim, K = *k, mode = *mask_mode;
        const bool self = train == nullptr;
        const int nt = self ? nq : (n_train ? *n_train : 0);
        if (nq < 1 || nt < 1) throw std::invalid_argument("n_query and n_train must be >= 1");
        if (d < 1) throw std::invalid_argument("dim must be >= 1");
        if (K < 1) throw std::invalid_argument("k must be >= 1");
        if (mode < 0 || mode > 2) throw std::invalid_argument("mask_mode must be 0 (none), 1 (exclude self) or 2 (exclude group)");
        if (mode != 0 && !self) throw std::invalid_argument("mask modes 1 and 2 need train = NULL (the query matrix itself)");
        if (!query || !out_idx || !out_dist) throw std::invalid_argument("null array");
        if ((long)*out_capacity < (long)nq * K) throw std::invalid_argument("out_capacity < n_query * k");
        std::vector<int> gk;
        if (mode == 2) {
            if (!group || !n_groups || *n_groups < 1) throw std::invalid_argument("mask mode 2 needs group and n_groups >= 1");
            for (int i = 0; i < nq; ++i)
                if (group[i] < 0 || group[i] >= *n_groups) throw std::invalid_argument("a group lies outside [0, n_groups)");
            if (group_k) {
                gk.assign(group_k, group_k + *n_groups);
                for (int v : gk)
                    if (v < 0 || v > K) throw std::invalid_argument("group_k must lie in [0, k]");
            }
        }
        HIPCHK(hipSetDevice(env_device()));
        Stream st;
        DevBuf Qb, Tb, Gb, Kb, Ib, Db;
        const float* dQ = upload<float>(Qb, query, (size_t)nq * d, st.s);
        const float* dT = self ? dQ : upload<float>(Tb, train, (size_t)nt * d, st.s);
        const int* dg = mode == 2 ? upload<int>(Gb, group, nq, st.s) : nullptr;
        const int* dk = gk.empty() ? nullptr : upload<int>(Kb, gk.data(), gk.size(), st.s);
        int* di = dalloc<int>(Ib, (size_t)nq * K);
        float* dd = dalloc<float>(Db, (size_t)nq * K);
        knn_device(dQ, nq, dT, nt, d, mode, dg, dk, K, K, di, dd, st.s);
        std::vector<int> hi((size_t)nq * K);
        std::vector<float> hd((size_t)nq * K);
        download<int>(hi.data(), di, hi.size(), st.s);
        download<float>(hd.data(), dd, hd.size(), st.s);
        std::copy(hi.begin(), hi.end(), out_idx);
        std::copy(hd.begin(), hd.end(), out_dist);
    });
}

extern "C" void rcppml_gpu_assess_plan(const int* labels, int* n, int* n_classes, int* kmeans_nstart, int* sil_samples_per_class,
                                       int* knn_folds, int* seed, int* out_init_idx, int* init_capacity, int* out_sil_samples,
                                       int* out_sil_counts, int* sil_capacity, int* out_fold_ids, int* fold_capacity, int* out_status) {
    entry_guard(out_status, [&] {
        if (!n || !n_classes || !seed) throw std::invalid_argument("null scalar argument");
        const int N = *n, nc = *n_classes;
        const unsigned sd = (unsigned)*seed;
        if (N < 1) throw std::invalid_argument("n must be >= 1");
        if (nc < 1) throw std::invalid_argument("n_classes must be >= 1");
        if (!labels) throw std::invalid_argument("null labels");
        for (int i = 0; i < N; ++i)
            if (labels[i] < 0 || labels[i] >= nc) throw std::invalid_argument("a label lies outside [0, n_classes)");
        std::vector<int> init, samples, counts, folds;
        if (out_init_idx) {
            if (!kmeans_nstart) throw std::invalid_argument("null kmeans_nstart");
            const int R = std::max(*kmeans_nstart, 0);
            need(true, init_capacity, (long)R * nc, "init_capacity");
            init.resize((size_t)R * nc);
            for (int r = 0; r < R; ++r) {
                const std::vector<int> one = kmeans_init(N, nc, 1, sd + (unsigned)r);
                std::copy(one.begin(), one.end(), init.begin() + (size_t)r * nc);
            }
        }
        if (out_sil_samples || out_sil_counts) {
            if (!sil_samples_per_class) throw std::invalid_argument("null sil_samples_per_class");
            sil_plan(labels, N, nc, *sil_samples_per_class, sd, samples, counts);
            if (out_sil_samples) need(true, sil_capacity, (long)samples.size(), "sil_capacity");
        }
        if (out_fold_ids) {
            if (!knn_folds || *knn_folds < 1) throw std::invalid_argument("knn_folds must be >= 1");
            need(true, fold_capacity, N, "fold_capacity");
            folds = fold_plan(labels, N, nc, *knn_folds, sd);
        }
        if (out_init_idx) std::copy(init.begin(), init.end(), out_init_idx);
        if (out_sil_samples) std::copy(samples.begin(), samples.end(), out_sil_samples);
        if (out_sil_counts) std::copy(counts.begin(), counts.end(), out_sil_counts);
        if (out_fold_ids) std::copy(folds.begin(), folds.end(), out_fold_ids);
    });
}
