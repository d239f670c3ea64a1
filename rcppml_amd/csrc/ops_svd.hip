// ops_svd.hip -- truncated SVD / PCA on the device (kernels: kernels_svd.hip.h) and the reference plugin's four entries
// rcppml_gpu_svd_pca_{double,float} (sparse CSC) and rcppml_gpu_svd_pca_dense_{double,float} (column-major dense), with the
// reference's pointer lists (src/gpu_bridge_svd.cu:53, 220, 392, 555) and the buffers R allocates (R/gpu_backend.R:295-420).
//
// algorithm 0: deflation, the reference's CPU deflation_svd (inst/include/FactorNet/svd/deflation.hpp:600-915) restated: SplitMix64
//   start (seed 0 -> 42), power-step warm start of later factors, Nesterov momentum, adaptive tol_k, L2 -> L1 -> nonneg -> upper
//   bound, two-pass Gram-Schmidt after each factor and a Rayleigh-quotient sigma, early stop when sigma ~ 0.  One iteration is five
//   launches (A'u, the v epilogue, A v, the u epilogue, the finish) with no host synchronisation; a converged factor freezes on the
//   device at the CPU's iteration and the host polls one flag every kPoll iterations.
// algorithms 1-4 without element constraints: Golub-Kahan-Lanczos with full two-pass reorthogonalisation (svd/lanczos.hpp); the
//   small bidiagonal problem is solved on the host in fp64.
// Anything else is refused (status -1, reason in rcppml_gpu_last_error, no output written).
//
// Cross-validation / auto-rank and obs_mask (deflation.hpp:431-565, :713-781, :869-896; kernels: kernels_svd_cv.hip.h) run through
// the build-defined entries rcppml_gpu_svd_cv_ex / rcppml_gpu_svd_cv_dense_ex at the end of this file, deflation only: the engine
// factors a training copy of A (held-out and masked values zeroed, same pattern), scales the two update denominators by the
// reference's correction, and after each stored factor updates the held-out residuals in one launch and applies the patience
// rule on the host, at the synchronisation the factor's sigma already needs.  The four reference entries keep refusing both.
//
// L21, angular and graph regularisation (deflation.hpp:191-292, :734-742, :779-787; kernels: kernels_svd_reg.hip.h) run through the
// build-defined entries rcppml_gpu_svd_reg_ex / rcppml_gpu_svd_reg_dense_ex, a superset of the cv entries: a side with a term on
// runs a chain of launches in place of its one epilogue, and with every term off the engine launches what the cv entries launch.
//
// The randomized block method (svd/randomized.hpp:59-241, Halko-Martinsson-Tropp; kernels: kernels_svd_rand.hip.h) runs through the
// build-defined entries rcppml_gpu_svd_randomized_ex / rcppml_gpu_svd_randomized_dense_ex: a fixed 2q + 2 block products against
// l = k + oversampling <= 128 vectors, CholeskyQR2 between them, and one host synchronisation for the l x l eigenproblem at the end.
// algorithm 3 on the four reference entries still runs Lanczos.
//
// The SVD-seeded start of an NMF fit (nmf/nmf_init.hpp:45-158; kernel: nmf_start_kernel in kernels_svd.hip.h) runs through the
// build-defined entries rcppml_gpu_nmf_svd_init_ex / rcppml_gpu_nmf_svd_init_dense_ex at the end of this file: Lanczos with the
// reference's fixed options in an output mode (Opts::nmf_start) that writes the Ritz product as W_T and H of the fit entries.
//
// Centering never densifies: A'u - (mu . u) 1 and A v - mu sum(v) are scalar corrections inside the epilogues.
//
// The host boundary of the fourteen SVD entries and the two NMF-start entries is written once (section "boundary"): load_shared() /
// load_checked() fill the fields of Opts every family shares and raise the shared refusals, attach_csc() / attach_dense() (with
// FullCsc for the block methods' dense entries) hand the matrix over, fit() checks the device and runs Engine<float> or
// Engine<double> under the clock, and write_shared() copies the outputs every family has.  A family adds its own pointer struct,
// make_*_opts, *_bytes and write_*.  Opts::method names what the engine runs; the reference entries' algorithm 1-4 become
// Method::lanczos at the boundary.
#include "entry_common.hip.h"
#include "kernels_svd.hip.h"
#include "kernels_svd_cv.hip.h"
#include "kernels_svd_krylov.hip.h"
#include "kernels_svd_rand.hip.h"
#include "kernels_svd_reg.hip.h"

#include <chrono>
#include <climits>
#include <limits>

namespace {
using namespace rcppml_plugin;
using namespace rsv;

constexpr int kPoll = 8;

int nblk(long len) { return (int)((len + CH - 1) / CH); }
int wblk(long len) { return (int)((len + NW - 1) / NW); }

// what Engine::run() runs; the reference entries' algorithm 1-4 are all lanczos
enum class Method { deflation, lanczos, kspr, randomized };

// the instantiation of a block kernel f<T, W> for w <= 128 columns: W sixteens, rounded up to a power of two
#define RSV_BY_WIDTH(f, w) ((w) <= 16 ? f<T, 1> : (w) <= 32 ? f<T, 2> : (w) <= 64 ? f<T, 4> : f<T, 8>)

struct Opts {
    int m, n, k;
    int64_t nnz;
    const int* p = nullptr; const int* i = nullptr; const double* x = nullptr;   // sparse CSC
    const double* dense = nullptr;                                              // or column-major dense
    double tol; int max_iter; int center; unsigned seed; Method method = Method::deflation;
    double L1_u, L1_v, L2_u, L2_v, ub_u, ub_v; int nonneg_u, nonneg_v;
    // the cv entries only: hold-out fraction (0: no CV), effective mask seed, patience, mask_zeros, obs-mask pattern CSC (or null)
    double test_fraction = 0; uint64_t cv_seed = 0; int patience = 0; int mask_zeros = 0;
    const int* mp = nullptr; const int* mi = nullptr; int64_t mnnz = 0;
    // the krylov entries only (Method::kspr): the pass limit (0: the default) and the n x k seed (null: Lanczos); max_iter stays 0.
    // The randomized entries (Method::randomized) add no field: max_iter is the block method's q (<= 0: 3)
    int ks_iter = 0; const double* V0 = nullptr;
    // the NMF-start entries only (Method::lanczos): the Ritz product leaves as W_T (k x m) and H (k x n) of nmf/nmf_init.hpp:71-90
    // in Result::U / V, and init_seed seeds the fill of the rows Lanczos did not deliver
    bool nmf_start = false; uint32_t init_seed = 0;
    // the reg entries only: L21 and angular per side, and a square graph CSC per side (p = null or lambda <= 0: none)
    double L21_u = 0, L21_v = 0, ang_u = 0, ang_v = 0;
    struct Graph {
        const int* p = nullptr; const int* i = nullptr; const double* x = nullptr; int dim = 0; int64_t nnz = 0; double lambda = 0;
        bool on() const { return p && lambda > 0 && nnz > 0; }     // an empty L is the identity step: nothing to launch
    } gu, gv;
    bool cv() const { return test_fraction > 0; }
    bool trains() const { return cv() || mp; }      // the products read a training copy of A
    // the products and block kernels read a CSC: the block methods read a dense matrix as a full CSC (KSPR's Lanczos seed still
    // runs the dense products)
    bool reads_csc() const { return !dense || method == Method::kspr || method == Method::randomized; }
};

struct Result {
    std::vector<double> U, V, d, row_means;
    std::vector<int> iters;
    int k_sel = 0;
    double frob = 0;
    std::vector<double> test_loss;          // one value per computed factor (CV only)
    int k_computed = 0, n_test = 0;
    int64_t n_masked = 0;
    int passes = 0;                         // KSPR: passes run, and the dW of each pass from the second on
    std::vector<double> dw;
};

bool has_constraints(const Opts& o) {
    return o.L1_u != 0 || o.L1_v != 0 || o.L2_u != 0 || o.L2_v != 0 || o.nonneg_u || o.nonneg_v || o.ub_u != 0 || o.ub_v != 0;
}

// ------------------------------------------------------------------------------------------------------------ host eigen
// Eigenvalues (d, ascending after sorting by the caller) and eigenvector rows of a symmetric tridiagonal matrix (diagonal d[0..n),
// off-diagonal e[1..n)) by implicit QL with shifts.  Z: zr rows x n, row-major, initialised by the caller (rows of the identity);
// every rotation is applied to those rows only, so tracking one row costs O(n^2) and all rows O(n^3).
void tql(std::vector<double>& d, std::vector<double> e, int n, std::vector<double>& Z, int zr) {
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    if (n > 0) e[n - 1] = 0.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < n - 1; ++mm) {
                const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
                if (std::fabs(e[mm]) <= std::numeric_limits<double>::epsilon() * dd) break;
            }
            if (mm != l) {
                if (++iter > 60) throw std::runtime_error("tridiagonal eigensolver did not converge");
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[mm] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    double f = s * e[i], b = c * e[i];
                    e[i + 1] = (r = std::hypot(f, g));
                    if (r == 0.0) { d[i + 1] -= p; e[mm] = 0.0; break; }
                    s = f / r; c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    d[i + 1] = g + (p = s * r);
                    g = c * r - b;
                    for (int z = 0; z < zr; ++z) {
                        double* row = &Z[(size_t)z * n];
                        f = row[i + 1];
                        row[i + 1] = s * row[i] + c * f;
                        row[i] = c * row[i] - s * f;
                    }
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p; e[l] = g; e[mm] = 0.0;
            }
        } while (mm != l);
    }
}

// SVD of the upper bidiagonal B (alpha on the diagonal, beta[1..ja) above it) through the eigenproblem of B'B:
// sigma descending, right vectors Vb (ja x ja, column-major), left vectors Ub = B Vb / sigma (zero columns for sigma = 0).
// rows_only: only the last row of Ub is wanted (the Ritz residual check): Vb is tracked in its last row only.
void bidiag_svd(const std::vector<double>& a, const std::vector<double>& b, int ja, std::vector<double>& sig, std::vector<double>& Ub,
                std::vector<double>& Vb, bool last_row_only) {
    std::vector<double> dd(ja), ee(ja, 0.0);
    for (int l = 0; l < ja; ++l) {
        dd[l] = a[l] * a[l] + (l > 0 ? b[l] * b[l] : 0.0);
        if (l > 0) ee[l] = a[l - 1] * b[l];
    }
    const int zr = last_row_only ? 1 : ja;
    std::vector<double> Z((size_t)zr * ja, 0.0);
    for (int z = 0; z < zr; ++z) Z[(size_t)z * ja + (last_row_only ? ja - 1 : z)] = 1.0;
    tql(dd, ee, ja, Z, zr);
    std::vector<int> ord(ja);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return dd[x] > dd[y]; });
    sig.assign(ja, 0.0);
    for (int c = 0; c < ja; ++c) sig[c] = std::sqrt(std::max(dd[ord[c]], 0.0));
    if (last_row_only) {                 // Ub(ja-1, c) = alpha_{ja-1} Vb(ja-1, c) / sigma_c  (the last row of B holds alpha only)
        Ub.assign(ja, 0.0);
        for (int c = 0; c < ja; ++c) Ub[c] = sig[c] > 0 ? a[ja - 1] * Z[ord[c]] / sig[c] : 0.0;
        return;
    }
    Vb.assign((size_t)ja * ja, 0.0);
    Ub.assign((size_t)ja * ja, 0.0);
    for (int c = 0; c < ja; ++c)
        for (int l = 0; l < ja; ++l) Vb[(size_t)c * ja + l] = Z[(size_t)l * ja + ord[c]];
    for (int c = 0; c < ja; ++c) {
        if (!(sig[c] > 0)) continue;
        const double* v = &Vb[(size_t)c * ja];
        for (int l = 0; l < ja; ++l) Ub[(size_t)c * ja + l] = (a[l] * v[l] + (l + 1 < ja ? b[l + 1] * v[l + 1] : 0.0)) / sig[c];
    }
}

// ------------------------------------------------------------------------------------------------------------ host QR / SVD
// KSPR's Phase 3 (krylov.hpp:216-247), once per call on k columns.
// A (rows x k, column-major) = Q R by twice-applied modified Gram-Schmidt: A becomes Q, R (k x k, column-major) is upper triangular.
// A column that vanishes leaves a zero column in Q and a zero on R's diagonal, so Q R = A still holds.
void mgs2_qr(std::vector<double>& A, int rows, int k, std::vector<double>& Rm) {
    Rm.assign((size_t)k * k, 0.0);
    for (int j = 0; j < k; ++j) {
        double* v = &A[(size_t)j * rows];
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < j; ++i) {
                const double* q = &A[(size_t)i * rows];
                double r = 0;
                for (int t = 0; t < rows; ++t) r += q[t] * v[t];
                for (int t = 0; t < rows; ++t) v[t] -= r * q[t];
                Rm[(size_t)j * k + i] += r;
            }
        double nn = 0;
        for (int t = 0; t < rows; ++t) nn += v[t] * v[t];
        nn = std::sqrt(nn);
        Rm[(size_t)j * k + j] = nn;
        for (int t = 0; t < rows; ++t) v[t] = nn > 0 ? v[t] / nn : 0.0;
    }
}
// S (k x k, column-major) = Us diag(sig) Vs' by one-sided Jacobi, sig descending (ties by index)
void jacobi_svd(std::vector<double> S, int k, std::vector<double>& Us, std::vector<double>& sig, std::vector<double>& Vs) {
    std::vector<double> Vm((size_t)k * k, 0.0);
    for (int c = 0; c < k; ++c) Vm[(size_t)c * k + c] = 1.0;
    const double eps = std::numeric_limits<double>::epsilon();
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < k - 1; ++p)
            for (int q = p + 1; q < k; ++q) {
                double* gp = &S[(size_t)p * k];
                double* gq = &S[(size_t)q * k];
                double al = 0, be = 0, ga = 0;
                for (int t = 0; t < k; ++t) { al += gp[t] * gp[t]; be += gq[t] * gq[t]; ga += gp[t] * gq[t]; }
                if (!(std::fabs(ga) > eps * std::sqrt(al * be))) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                double* vp = &Vm[(size_t)p * k];
                double* vq = &Vm[(size_t)q * k];
                for (int r = 0; r < k; ++r) {
                    const double a = gp[r], b = gq[r];
                    gp[r] = c * a - sn * b; gq[r] = sn * a + c * b;
                    const double x = vp[r], y = vq[r];
                    vp[r] = c * x - sn * y; vq[r] = sn * x + c * y;
                }
            }
        if (!rotated) break;
    }
    std::vector<double> nrm(k);
    for (int c = 0; c < k; ++c) {
        double s = 0;
        for (int t = 0; t < k; ++t) s += S[(size_t)c * k + t] * S[(size_t)c * k + t];
        nrm[c] = std::sqrt(s);
    }
    std::vector<int> ord(k);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return nrm[x] > nrm[y]; });
    Us.assign((size_t)k * k, 0.0); Vs.assign((size_t)k * k, 0.0); sig.assign(k, 0.0);
    for (int c = 0; c < k; ++c) {
        const int s = ord[c];
        sig[c] = nrm[s];
        for (int t = 0; t < k; ++t) {
            Us[(size_t)c * k + t] = nrm[s] > 0 ? S[(size_t)s * k + t] / nrm[s] : 0.0;
            Vs[(size_t)c * k + t] = Vm[(size_t)s * k + t];
        }
    }
}
// out (rows x k) = Q (rows x k) M (k x k), all column-major
std::vector<double> times_small(const std::vector<double>& Q, int rows, int k, const std::vector<double>& M) {
    std::vector<double> out((size_t)rows * k, 0.0);
    for (int c = 0; c < k; ++c)
        for (int l = 0; l < k; ++l) {
            const double w = M[(size_t)c * k + l];
            const double* q = &Q[(size_t)l * rows];
            double* y = &out[(size_t)c * rows];
            for (int t = 0; t < rows; ++t) y[t] += q[t] * w;
        }
    return out;
}

// svd/lanczos.hpp: jmax = min(min(m, n) - 1, max(3k, k + 50, max_iter)); k = min(m, n) may use all min(m, n) steps.  Throws when the
// partial columns of jmax + 1 steps would not fit a consumer's LDS.
int lanczos_steps(int m, int n, int K, int max_iter) {
    const int mn = std::min(m, n);
    const int cap = K >= mn ? mn : mn - 1;
    const int jmax = std::min(cap, std::max(std::max(3 * K, K + 50), max_iter > 0 ? max_iter : 0));
    if (jmax + 1 > NPMAX) throw std::invalid_argument("Lanczos would need more than " + std::to_string(NPMAX - 1) + " steps");
    return jmax;
}

// ------------------------------------------------------------------------------------------------------------ engine
template <class T> struct Engine {
    const Opts& o;
    CtxGuard g;
    hipStream_t s;
    int m, n;
    DevBuf Ap, Ai, Ax, Tp, Ti, Tx, Ad, mu;
    DevBuf Xt, Mp, Mi, te_rows, te_cols, te_res, te_P;      // training values (CSC order or dense), obs-mask, test entries
    long n_test = 0;
    int64_t n_masked = 0;
    std::vector<double> mu_h;
    struct DevGraph { DevBuf p, i, x, tp, ti, tx; } Gu, Gv;      // a graph and its rows (the CSC of L')

    Engine(const Opts& o_) : o(o_), g(env_device()), s(g.s), m(o_.m), n(o_.n) {
        mu_h.assign(m, 0.0);
        if (o.dense) {
            if (o.method != Method::randomized) upload_cast<T>(g.c, o.dense, (size_t)m * n, Ad, s);
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < m; ++i) mu_h[i] += o.dense[(size_t)j * m + i];
        }
        if (o.reads_csc()) {
            const size_t nz = (size_t)std::max<int64_t>(o.nnz, 1);
            upload_ints(o.p, (size_t)n + 1, Ap, s);
            upload_ints(o.i, nz, Ai, s);
            upload_cast<T>(g.c, o.x, nz, Ax, s);
            if (!o.dense)
                for (int64_t e = 0; e < o.nnz; ++e) mu_h[o.i[e]] += o.x[e];
        }
        for (auto& v : mu_h) v /= (double)n;
        if (o.center) {
            std::vector<double> tmp(mu_h);
            upload_cast<T>(g.c, tmp.data(), (size_t)m, mu, s);
        }
        if (o.trains()) hold_out();
        if (o.reads_csc()) {
            const size_t nz = (size_t)std::max<int64_t>(o.nnz, 1);
            grow<int>(Tp, (size_t)m + 1);
            grow<int>(Ti, nz);
            grow<T>(Tx, nz);
            OPCHK(rcppml_hip_transpose_csc(g.c, DT<T>::id, m, n, Ap.as<int>(), Ai.as<int>(),
                                           (const void*)(o.trains() ? Xt.as<T>() : Ax.as<T>()), Tp.as<int>(), Ti.as<int>(), Tx.p));
        }
        if (o.gu.on()) upload_graph(o.gu, Gu);
        if (o.gv.on()) upload_graph(o.gv, Gv);
    }
    void upload_graph(const Opts::Graph& gr, DevGraph& G) {
        upload_ints(gr.p, (size_t)gr.dim + 1, G.p, s);
        upload_ints(gr.i, (size_t)gr.nnz, G.i, s);
        upload_cast<T>(g.c, gr.x, (size_t)gr.nnz, G.x, s);
        grow<int>(G.tp, (size_t)gr.dim + 1);
        grow<int>(G.ti, (size_t)gr.nnz);
        grow<T>(G.tx, (size_t)gr.nnz);
        OPCHK(rcppml_hip_transpose_csc(g.c, DT<T>::id, gr.dim, gr.dim, (const int*)G.p.p, (const int*)G.i.p, (const void*)G.x.p,
                                       (int*)G.tp.p, (int*)G.ti.p, G.tx.p));
    }
    const T* mup() const { return o.center ? mu.as<T>() : nullptr; }
    // the values the products read: the training copy when there is one
    const T* xa() const { return o.trains() ? Xt.as<T>() : (o.dense ? Ad.as<T>() : Ax.as<T>()); }
    // The test entries from the original A (row means subtracted when centred) and the training values, deflation.hpp:452-545.
    void hold_out() {
        const uint64_t thr = o.cv() ? UINT64_MAX / (uint64_t)(1.0 / o.test_fraction) : 0;
        const int* p = o.dense ? nullptr : Ap.as<int>();
        const int* ri = o.dense ? nullptr : Ai.as<int>();
        const T* x = o.dense ? Ad.as<T>() : Ax.as<T>();
        const size_t len = o.dense ? (size_t)m * n : (size_t)std::max<int64_t>(o.nnz, 1);
        DevBuf cnt, off;
        int* dcnt = grow<int>(cnt, (size_t)n);
        if (o.cv()) {
            hipLaunchKernelGGL(test_entries<T>, dim3(wblk(n)), dim3(WG), 0, s, p, ri, x, m, n, (unsigned long long)o.cv_seed,
                               (unsigned long long)thr, mup(), (const int*)nullptr, dcnt, (int*)nullptr, (int*)nullptr, (T*)nullptr);
            HIPCHK(hipGetLastError());
            const std::vector<int> ch = read<int>(dcnt, (size_t)n);
            std::vector<int> oh((size_t)n + 1, 0);
            int64_t tot = 0;
            for (int j = 0; j < n; ++j) { oh[j] = (int)tot; tot += ch[j]; if (tot >= INT_MAX) throw std::invalid_argument("too many test entries"); }
            oh[n] = (int)tot;
            n_test = (long)tot;
            upload_ints(oh.data(), (size_t)n + 1, off, s);
            grow<int>(te_rows, (size_t)std::max<long>(n_test, 1));
            grow<int>(te_cols, (size_t)std::max<long>(n_test, 1));
            grow<T>(te_res, (size_t)std::max<long>(n_test, 1));
            grow<T>(te_P, (size_t)std::max(nblk(n_test), 1));
            if (n_test > 0)
                hipLaunchKernelGGL(test_entries<T>, dim3(wblk(n)), dim3(WG), 0, s, p, ri, x, m, n, (unsigned long long)o.cv_seed,
                                   (unsigned long long)thr, mup(), (const int*)off.as<int>(), (int*)nullptr, te_rows.as<int>(),
                                   te_cols.as<int>(), te_res.as<T>());
        }
        if (o.mp) {
            upload_ints(o.mp, (size_t)n + 1, Mp, s);
            upload_ints(o.mi, (size_t)std::max<int64_t>(o.mnnz, 1), Mi, s);
        }
        grow<T>(Xt, len);
        hipLaunchKernelGGL(train_values<T>, dim3(wblk(n)), dim3(WG), 0, s, p, ri, x, m, n, (unsigned long long)o.cv_seed,
                           (unsigned long long)thr, o.mp ? (const int*)Mp.as<int>() : nullptr, o.mp ? (const int*)Mi.as<int>() : nullptr,
                           Xt.as<T>(), dcnt);
        HIPCHK(hipGetLastError());
        const std::vector<int> mh = read<int>(dcnt, (size_t)n);      // also orders the off / cnt buffers' release after the kernels
        n_masked = 0;
        for (int c : mh) n_masked += c;
    }
    // y = A' x (n);  brk: a state word that skips the launch when set (0: none)
    void at(const T* x, T* y, const int* st, int it, int brk) {
        if (o.dense)
            hipLaunchKernelGGL(spmv_t_dense<T>, dim3(wblk(n)), dim3(WG), 0, s, xa(), m, n, x, y, st, it, brk);
        else
            hipLaunchKernelGGL(spmv_t_csc<T>, dim3(wblk(n)), dim3(WG), 0, s, Ap.as<int>(), Ai.as<int>(), xa(), n, x, y, st, it, brk);
    }
    // y = A x (m)
    void ax(const T* x, T* y, const int* st, int it, int brk) {
        if (o.dense)
            hipLaunchKernelGGL(spmv_dense<T>, dim3((m + WG - 1) / WG), dim3(WG), 0, s, xa(), m, n, x, y, st, it, brk);
        else
            hipLaunchKernelGGL(spmv_csr<T>, dim3(wblk(m)), dim3(WG), 0, s, Tp.as<int>(), Ti.as<int>(), Tx.as<T>(), m, x, y, st, it, brk);
    }
    void dots(const T* x, long len, const Cols<T>& C, T* P) {
        hipLaunchKernelGGL(dots_kernel<T>, dim3(nblk(len)), dim3(WG), 0, s, x, len, C, P);
    }
    template <class X> std::vector<X> read(const void* src, size_t count) {
        std::vector<X> h(count);
        HIPCHK(hipMemcpyAsync(h.data(), src, count * sizeof(X), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return h;
    }

    // -------------------------------------------------------------------------------------------------------- deflation
    void deflation(Result& R) {
        const int K = o.k, nbm = nblk(m), nbn = nblk(n);
        const T eps100 = std::numeric_limits<T>::epsilon() * T(100);
        const T l1u = (T)o.L1_u, l1v = (T)o.L1_v, l2u = (T)o.L2_u, l2v = (T)o.L2_v, ubu = (T)o.ub_u, ubv = (T)o.ub_v;
        // deflation.hpp:552-559: the denominators |u_hat|^2 and |v|^2 count the held-out positions too
        T dc = T(1);
        if (o.cv()) dc = T(1) - (T)o.test_fraction * (o.mask_zeros ? (T)o.nnz / ((T)m * (T)n) : T(1));
        T best = std::numeric_limits<T>::max();
        int best_k = 0, waited = 0;
        R.test_loss.clear();
        DevBuf dU, dV, dd, uraw, uhat, vraw, y, t, Pm, Pn, Pu, st, nrm;
        T* U = grow<T>(dU, (size_t)m * K);
        T* V = grow<T>(dV, (size_t)n * K);
        T* d = grow<T>(dd, K);
        grow<T>(uraw, m); grow<T>(uhat, m); grow<T>(vraw, n); grow<T>(y, n); grow<T>(t, m);
        grow<T>(Pm, (size_t)nbm * (K + 2)); grow<T>(Pn, (size_t)nbn * (K + 2)); grow<T>(Pu, (size_t)nbm * 2);
        int* S = grow<int>(st, S_WORDS);
        T* dn = grow<T>(nrm, 1);
        // kernels_svd_reg.hip.h: a side with L21, angular (from the second factor on) or a graph runs a chain instead of its epilogue
        const T l21u = (T)o.L21_u, l21v = (T)o.L21_v, angu = (T)o.ang_u, angv = (T)o.ang_v;
        const bool any_reg = l21u > 0 || l21v > 0 || angu > 0 || angv > 0 || o.gu.on() || o.gv.on();
        DevBuf bQa, bQb, bnsq, blx;
        T *Qa = nullptr, *Qb = nullptr, *nsq = nullptr, *lx = nullptr;
        if (any_reg) {
            Qa = grow<T>(bQa, (size_t)std::max(nbm, nbn) * (K + 2));
            Qb = grow<T>(bQb, (size_t)std::max(nbm, nbn) * (K + 2));
            nsq = grow<T>(bnsq, 2);
            lx = grow<T>(blx, (size_t)std::max(m, n));
        }
        // the links after a head, on x (len) in place: the head left the mid partials (k + 2 columns, |x|^2 in column sq) in Qa;
        // the last link writes Cfin -> Pfin
        auto chain = [&](T* x, long len, int nb, const T* F, int kf, int sq, T l1, T l2, T l21, int nonneg, T ub, T ang,
                         const Opts::Graph& gr, const DevGraph& G, const T* nq, const Cols<T>& Cmid, const Cols<T>& Cfin, T* Pfin, int it,
                         int uside) {
            const bool on[3] = {l21 > 0, ang > 0 && kf > 0, gr.on()};
            const int last = on[2] ? 2 : on[1] ? 1 : 0;
            const T* Pin = Qa;
            for (int op = 0; op < 3; ++op) {
                if (!on[op]) continue;
                T* Pout = op == last ? Pfin : (Pin == Qa ? Qb : Qa);
                const Cols<T>& Co = op == last ? Cfin : Cmid;
                if (op == 0)
                    hipLaunchKernelGGL(reg_shrink_kernel<T>, dim3(nb), dim3(WG), 0, s, x, len, Pin, nb, kf + 2, sq, nq, l1, l2, l21, nonneg, ub,
                                       Co, Pout, (const int*)S, it, uside);
                else if (op == 1)
                    hipLaunchKernelGGL(reg_angular_kernel<T>, dim3(nb), dim3(WG), 0, s, x, len, F, kf, Pin, nb, kf + 2, nq, ang, Co, Pout,
                                       (const int*)S, it, uside);
                else {
                    hipLaunchKernelGGL(spmv_csr<T>, dim3(wblk(len)), dim3(WG), 0, s, (const int*)G.tp.p, (const int*)G.ti.p, (const T*)G.tx.p, (int)len, (const T*)x, lx,
                                       (const int*)S, it, uside ? (int)S_BRKU : (int)S_BRKV);
                    hipLaunchKernelGGL(reg_graph_kernel<T>, dim3(nb), dim3(WG), 0, s, x, len, (const T*)lx, nq, (T)gr.lambda, Co, Pout,
                                       (const int*)S, it, uside);
                }
                Pin = Pout;
            }
        };
        HIPCHK(hipMemsetAsync(U, 0, (size_t)m * K * sizeof(T), s));
        HIPCHK(hipMemsetAsync(V, 0, (size_t)n * K * sizeof(T), s));
        HIPCHK(hipMemsetAsync(d, 0, (size_t)K * sizeof(T), s));
        const uint64_t seed = o.seed == 0 ? 42ull : (uint64_t)o.seed;
        uint64_t drawn = 0;
        std::vector<T> dh(K, T(0));
        const int init[S_WORDS] = {INT_MAX, 0, 0, 0, 0, 0, 0, 0};
        auto random_u = [&](T* u) {        // the next m uniform<double>() draws, cast to the working precision
            const std::vector<double> r = splitmix<double>(seed, drawn, (size_t)m);
            drawn += m;
            std::vector<T> rt(r.begin(), r.end());
            HIPCHK(hipMemcpyAsync(u, rt.data(), (size_t)m * sizeof(T), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        };
        R.iters.clear();
        int k = 0;
        for (; k < K; ++k) {
            T* u = U + (size_t)k * m;
            T* v = V + (size_t)k * n;
            Cols<T> Cm;                                         // m side: [U_k' x, mu . x (or sum), |x|^2]
            Cm.X = U; Cm.ld = m; Cm.nx = k; Cm.e[0] = mup(); Cm.ne = 2;
            Cols<T> Cn;                                         // n side: [V_k' x, sum x, |x|^2]
            Cn.X = V; Cn.ld = n; Cn.nx = k; Cn.e[0] = nullptr; Cn.ne = 2;
            // ---- start vector
            bool rnd = k == 0;
            if (k > 0) {
                HIPCHK(hipMemcpyAsync(u, U + (size_t)(k - 1) * m, (size_t)m * sizeof(T), hipMemcpyDeviceToDevice, s));
                hipLaunchKernelGGL(gs_kernel<T>, dim3(1), dim3(WG), 0, s, u, (long)m, (const T*)U, k, 1, eps100, dn);
                const T ni = read<T>(dn, 1)[0];
                if (ni > eps100) {                              // power step: v = normalise(R' u), u = R v, MGS
                    Cm.e[1] = u;
                    dots(u, m, Cm, Pm.as<T>());
                    at(u, y.as<T>(), nullptr, 0, 0);
                    hipLaunchKernelGGL(defl_v_kernel<T>, dim3(nbn), dim3(WG), 0, s, (const T*)y.as<T>(), n, (const T*)V, k, (const T*)d,
                                       (const T*)Pm.as<T>(), nbm, o.center, T(0), T(0), 0, T(0), T(1), (int)M_WARM, vraw.as<T>(),
                                       Pn.as<T>(), (int*)nullptr, 0);
                    ax(vraw.as<T>(), t.as<T>(), nullptr, 0, 0);
                    hipLaunchKernelGGL(defl_u_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)t.as<T>(), m, (const T*)U, k, (const T*)d,
                                       (const T*)Pn.as<T>(), nbn, mup(), T(0), T(0), 0, T(0), T(1), (int)M_WARM, (const T*)vraw.as<T>(), v, n,
                                       u, (const T*)nullptr, Pu.as<T>(), (int*)nullptr, 0);
                    hipLaunchKernelGGL(gs_kernel<T>, dim3(1), dim3(WG), 0, s, u, (long)m, (const T*)U, k, 1, T(0), (T*)nullptr);
                } else {
                    rnd = true;
                }
            }
            if (rnd) {
                random_u(u);
                hipLaunchKernelGGL(gs_kernel<T>, dim3(1), dim3(WG), 0, s, u, (long)m, (const T*)nullptr, 0, 1, T(0), (T*)nullptr);
            }
            // ---- adaptive tolerance
            T tol_k = (T)o.tol;
            if (k > 0 && dh[0] > 0 && dh[k - 1] > 0) tol_k = std::min((T)o.tol * dh[0] / dh[k - 1], (T)o.tol * T(100));
            // ---- ALS iterations
            HIPCHK(hipMemcpyAsync(uhat.p, u, (size_t)m * sizeof(T), hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemcpyAsync(S, init, sizeof(init), hipMemcpyHostToDevice, s));
            Cm.e[1] = uhat.as<T>();
            dots(uhat.as<T>(), m, Cm, Pm.as<T>());
            // the regularised chains of this factor: angular has nothing to subtract from at k = 0
            const bool reg_v = l21v > 0 || (angv > 0 && k > 0) || o.gv.on(), reg_u = l21u > 0 || (angu > 0 && k > 0) || o.gu.on();
            Cols<T> Cnr = Cn, Cum, Cuf;                         // n side (mid = final); m side mid [U_k' x, |x|^2, x . u] and final
            Cnr.e[1] = vraw.as<T>();
            Cum.X = U; Cum.ld = m; Cum.nx = k; Cum.e[0] = uraw.as<T>(); Cum.e[1] = u; Cum.ne = 2;
            Cuf.e[0] = uraw.as<T>(); Cuf.e[1] = u; Cuf.ne = 2;
            for (int done = 0; done < o.max_iter;) {
                const int P = std::min(kPoll, o.max_iter - done);
                for (int q = 0; q < P; ++q) {
                    const int it = done + q;
                    at(uhat.as<T>(), y.as<T>(), S, it, 0);
                    if (!reg_v)
                        hipLaunchKernelGGL(defl_v_kernel<T>, dim3(nbn), dim3(WG), 0, s, (const T*)y.as<T>(), n, (const T*)V, k, (const T*)d,
                                           (const T*)Pm.as<T>(), nbm, o.center, l1v, l2v, o.nonneg_v, ubv, dc, (int)M_LOOP, vraw.as<T>(),
                                           Pn.as<T>(), S, it);
                    else {
                        hipLaunchKernelGGL(reg_v_head_kernel<T>, dim3(nbn), dim3(WG), 0, s, (const T*)y.as<T>(), n, (const T*)V, k,
                                           (const T*)d, (const T*)Pm.as<T>(), nbm, o.center, l1v, l2v, o.nonneg_v, ubv, dc,
                                           l21v > 0 ? 0 : 1, vraw.as<T>(), Qa, nsq, S, it);
                        chain(vraw.as<T>(), (long)n, nbn, (const T*)V, k, k + 1, l1v, l2v, l21v, o.nonneg_v, ubv, angv, o.gv, Gv,
                              (const T*)nsq, Cnr, Cnr, Pn.as<T>(), it, 0);
                    }
                    ax(vraw.as<T>(), t.as<T>(), S, it, S_BRKV);
                    if (!reg_u)
                        hipLaunchKernelGGL(defl_u_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)t.as<T>(), m, (const T*)U, k, (const T*)d,
                                           (const T*)Pn.as<T>(), nbn, mup(), l1u, l2u, o.nonneg_u, ubu, dc, (int)M_LOOP,
                                           (const T*)vraw.as<T>(), v, n, uraw.as<T>(), (const T*)u, Pu.as<T>(), S, it);
                    else {
                        hipLaunchKernelGGL(reg_u_head_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)t.as<T>(), m, (const T*)U, k,
                                           (const T*)d, (const T*)Pn.as<T>(), nbn, mup(), l1u, l2u, o.nonneg_u, ubu, dc, l21u > 0 ? 0 : 1,
                                           (const T*)vraw.as<T>(), v, n, uraw.as<T>(), (const T*)u, Qa, nsq + 1, S, it);
                        chain(uraw.as<T>(), (long)m, nbm, (const T*)U, k, k, l1u, l2u, l21u, o.nonneg_u, ubu, angu, o.gu, Gu,
                              (const T*)(nsq + 1), Cum, Cuf, Pu.as<T>(), it, 1);
                    }
                    hipLaunchKernelGGL(defl_finish_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)uraw.as<T>(), u, uhat.as<T>(), m,
                                       (const T*)Pu.as<T>(), nbm, (const T*)U, k, mup(), Pm.as<T>(), tol_k, S, it);
                }
                HIPCHK(hipGetLastError());
                done += P;
                if (read<int>(S + S_STOP, 1)[0] <= done) break;
            }
            const int iters = read<int>(S + S_ITERS, 1)[0];
            R.iters.push_back(iters);
            // ---- two-pass Gram-Schmidt against the earlier factors, then the Rayleigh quotient
            if (k > 0) {
                hipLaunchKernelGGL(gs_kernel<T>, dim3(1), dim3(WG), 0, s, u, (long)m, (const T*)U, k, 0, eps100, (T*)nullptr);
                hipLaunchKernelGGL(gs_kernel<T>, dim3(1), dim3(WG), 0, s, v, (long)n, (const T*)V, k, 0, eps100, (T*)nullptr);
            }
            Cn.e[1] = v;
            dots(v, n, Cn, Pn.as<T>());
            ax(v, t.as<T>(), nullptr, 0, 0);
            hipLaunchKernelGGL(defl_u_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)t.as<T>(), m, (const T*)U, k, (const T*)d,
                               (const T*)Pn.as<T>(), nbn, mup(), T(0), T(0), 0, T(0), T(1), (int)M_PLAIN, (const T*)v, (T*)nullptr, n,
                               uraw.as<T>(), (const T*)u, Pu.as<T>(), (int*)nullptr, 0);
            HIPCHK(hipGetLastError());
            const std::vector<T> pu = read<T>(Pu.p, (size_t)nbm * 2);
            T sg = 0;
            for (int b = 0; b < nbm; ++b) sg += pu[(size_t)b * 2 + 1];
            if (sg < 0) sg = -sg;
            dh[k] = sg;
            HIPCHK(hipMemcpyAsync(d + k, &dh[k], sizeof(T), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
            if (o.cv()) {                                       // deflation.hpp:869-896
                T mse = 0;
                if (n_test > 0) {
                    const int nbt = nblk(n_test);
                    hipLaunchKernelGGL(test_loss<T>, dim3(nbt), dim3(WG), 0, s, (const int*)te_rows.as<int>(), (const int*)te_cols.as<int>(),
                                       te_res.as<T>(), n_test, (const T*)u, (const T*)v, sg, te_P.as<T>());
                    HIPCHK(hipGetLastError());
                    const std::vector<T> pt = read<T>(te_P.p, (size_t)nbt);
                    for (int b = 0; b < nbt; ++b) mse += pt[b];
                    mse /= (T)n_test;
                }
                R.test_loss.push_back((double)mse);
                if (mse < best) { best = mse; best_k = k + 1; waited = 0; }
                else if (++waited >= o.patience) { ++k; break; }
            } else {
                best_k = k + 1;
            }
            if (sg < eps100) { ++k; break; }
        }
        R.k_computed = std::min(k, K);
        R.k_sel = best_k;
        R.U.resize((size_t)m * R.k_sel);
        R.V.resize((size_t)n * R.k_sel);
        download_cast<T>(g.c, dU, (size_t)m * R.k_sel, R.U.data(), s);
        download_cast<T>(g.c, dV, (size_t)n * R.k_sel, R.V.data(), s);
        R.d.assign(dh.begin(), dh.begin() + R.k_sel);
    }

    // -------------------------------------------------------------------------------------------------------- Lanczos
    void lanczos(Result& R) {
        const int K = o.k;
        const int jmax = lanczos_steps(m, n, K, o.max_iter);
        const int nbm = nblk(m), nbn = nblk(n);
        const T eps = std::numeric_limits<T>::epsilon() * T(100);
        const double conv_tol = o.tol > 0 ? o.tol : 1e-10;
        DevBuf dP, dQ, dal, dbe, r, sv, y, t, Pa, Pb, Pc, st;
        T* Pm = grow<T>(dP, (size_t)n * (jmax + 1));
        T* Q = grow<T>(dQ, (size_t)m * std::max(jmax, 1));
        T* al = grow<T>(dal, (size_t)jmax + 1);
        T* be = grow<T>(dbe, (size_t)jmax + 1);
        grow<T>(r, m); grow<T>(sv, n); grow<T>(y, n); grow<T>(t, m);
        const size_t pcap = (size_t)std::max(nbm, nbn) * (jmax + 2);
        grow<T>(Pa, pcap); grow<T>(Pb, pcap); grow<T>(Pc, pcap);
        int* S = grow<int>(st, S_WORDS);
        const int init[S_WORDS] = {INT_MAX, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(S, init, sizeof(init), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(be, 0, ((size_t)jmax + 1) * sizeof(T), s));
        {   // p0 = normalise(uniform<Scalar>() - 0.5)
            std::vector<T> p0 = splitmix<T>(o.seed == 0 ? 42ull : (uint64_t)o.seed, 0, (size_t)n);
            T nn = 0;
            for (auto& v : p0) { v -= T(0.5); nn += v * v; }
            nn = std::sqrt(nn);
            if (nn > 0) for (auto& v : p0) v /= nn;
            HIPCHK(hipMemcpyAsync(Pm, p0.data(), (size_t)n * sizeof(T), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        Cols<T> Csum;
        Csum.e[0] = nullptr; Csum.ne = 1;
        if (o.center) dots(Pm, n, Csum, Pc.as<T>());
        T* Psum = Pc.as<T>();                 // partials of sum(p_j), consumed by lz_r of step j
        DevBuf Pc2; T* Psum_next = grow<T>(Pc2, pcap);
        auto host_ab = [&](int ja, std::vector<double>& a, std::vector<double>& b) {
            const std::vector<T> ah = read<T>(al, (size_t)std::max(ja, 1)), bh = read<T>(be, (size_t)ja + 1);
            a.assign(ah.begin(), ah.begin() + ja);
            b.assign(bh.begin(), bh.begin() + ja + 1);
        };
        int j = 0;
        for (; j < jmax; ++j) {
            ax(Pm + (size_t)j * n, t.as<T>(), S, j, 0);
            hipLaunchKernelGGL(lz_r_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)t.as<T>(), m, mup(), (const T*)Psum, nbn, (const T*)be,
                               (const T*)Q, j, r.as<T>(), Pa.as<T>(), (const int*)S);
            const T* Pr = Pa.as<T>();
            if (j > 0) {
                hipLaunchKernelGGL(cgs_kernel<T>, dim3(nbm), dim3(WG), 0, s, r.as<T>(), (long)m, (const T*)Q, j, Pr, nbm, 0, Pb.as<T>(),
                                   (const int*)S, j, 0);
                hipLaunchKernelGGL(cgs_kernel<T>, dim3(nbm), dim3(WG), 0, s, r.as<T>(), (long)m, (const T*)Q, j, (const T*)Pb.as<T>(), nbm,
                                   1, Pa.as<T>(), (const int*)S, j, 0);
            }
            hipLaunchKernelGGL(lz_norm_kernel<T>, dim3(nbm), dim3(WG), 0, s, (const T*)r.as<T>(), (long)m, Pr, nbm, eps, (const T*)al, Q + (size_t)j * m,
                               al, j, 0, o.center, mup(), Pb.as<T>(), S, j);
            at(Q + (size_t)j * m, y.as<T>(), S, j, S_BRKV);
            hipLaunchKernelGGL(lz_s_kernel<T>, dim3(nbn), dim3(WG), 0, s, (const T*)y.as<T>(), n, (const T*)Pb.as<T>(), nbm, o.center,
                               (const T*)al, (const T*)Pm, j, sv.as<T>(), Pa.as<T>(), (const int*)S);
            hipLaunchKernelGGL(cgs_kernel<T>, dim3(nbn), dim3(WG), 0, s, sv.as<T>(), (long)n, (const T*)Pm, j + 1, (const T*)Pa.as<T>(), nbn,
                               0, Pb.as<T>(), (const int*)S, j, 1);
            hipLaunchKernelGGL(cgs_kernel<T>, dim3(nbn), dim3(WG), 0, s, sv.as<T>(), (long)n, (const T*)Pm, j + 1, (const T*)Pb.as<T>(), nbn,
                               1, Pa.as<T>(), (const int*)S, j, 1);
            hipLaunchKernelGGL(lz_norm_kernel<T>, dim3(nbn), dim3(WG), 0, s, (const T*)sv.as<T>(), (long)n, (const T*)Pa.as<T>(), nbn, eps, (const T*)al,
                               Pm + (size_t)(j + 1) * n, be, j + 1, 1, o.center, (const T*)nullptr, Psum_next, S, j);
            HIPCHK(hipGetLastError());
            std::swap(Psum, Psum_next);
            const int ja = j + 1;
            const bool check = ja >= K + 2 && ja % 5 == 0 && ja < jmax;
            if (!check && ja % kPoll != 0) continue;
            if (read<int>(S + S_STOP, 1)[0] <= ja) break;               // lucky breakdown
            if (!check) continue;
            std::vector<double> a, b, sig, ub, vb;
            host_ab(ja, a, b);
            bidiag_svd(a, b, ja, sig, ub, vb, true);
            const int kc = std::min(K, ja);
            const double bl = std::fabs(b[ja]);
            bool all = true;
            for (int c = 0; c < kc && all; ++c)
                if (bl * std::fabs(ub[c]) > conv_tol * sig[0]) all = false;
            if (all) break;
        }
        const int ja = read<int>(S + S_ITERS, 1)[0];
        const bool abrk = read<int>(S + S_BRKV, 1)[0] != 0;
        R.iters.assign(1, ja);
        const int kc = std::min(K, ja);
        R.k_sel = kc;
        R.d.clear(); R.U.clear(); R.V.clear();
        if (kc == 0) {
            if (o.nmf_start) nmf_start(R, nullptr, nullptr, 0, 0, {}, {}, {});
            return;
        }
        // An alpha breakdown at step ja (A p_ja in span Q) leaves beta_ja coupling p_ja: A [P_ja p_ja] = Q_ja [B_ja | beta_ja e],
        // so the small problem is the (ja + 1)-column bidiagonal with a trailing alpha = 0 (its extra singular value is 0 and the
        // last row of its left vectors vanishes).  svd/lanczos.hpp drops beta_ja there, which is wrong on low-rank input.
        const int nbd = abrk ? ja + 1 : ja;
        std::vector<double> a, b, sig, Ub, Vb;
        host_ab(ja, a, b);
        if (abrk) { a.push_back(0.0); b.push_back(0.0); }
        bidiag_svd(a, b, nbd, sig, Ub, Vb, false);
        R.d.assign(sig.begin(), sig.begin() + kc);
        std::vector<T> wu((size_t)ja * kc), wv((size_t)nbd * kc);
        for (int c = 0; c < kc; ++c) {
            for (int l = 0; l < ja; ++l) wu[(size_t)c * ja + l] = (T)Ub[(size_t)c * nbd + l];
            for (int l = 0; l < nbd; ++l) wv[(size_t)c * nbd + l] = (T)Vb[(size_t)c * nbd + l];
        }
        if (o.nmf_start) {
            nmf_start(R, Q, Pm, ja, nbd, wu, wv, sig);
            return;
        }
        DevBuf dwu, dwv, ou, ov;
        upload_vec(wu, dwu);
        upload_vec(wv, dwv);
        grow<T>(ou, (size_t)m * kc); grow<T>(ov, (size_t)n * kc);
        hipLaunchKernelGGL(ritz_kernel<T>, dim3((m + WG - 1) / WG, kc), dim3(WG), 0, s, (const T*)Q, (long)m, ja, (const T*)dwu.as<T>(), kc,
                           ou.as<T>());
        hipLaunchKernelGGL(ritz_kernel<T>, dim3((n + WG - 1) / WG, kc), dim3(WG), 0, s, (const T*)Pm, (long)n, nbd, (const T*)dwv.as<T>(), kc,
                           ov.as<T>());
        HIPCHK(hipGetLastError());
        R.U.resize((size_t)m * kc);
        R.V.resize((size_t)n * kc);
        download_cast<T>(g.c, ou, (size_t)m * kc, R.U.data(), s);
        download_cast<T>(g.c, ov, (size_t)n * kc, R.V.data(), s);
    }
    // The output mode of the NMF-start entries, in place of the two ritz_kernel launches: R.U = W_T (k x m column-major) with
    // W_T(c, i) = |u_c(i)| sqrt(sigma_c) and R.V = H (k x n) likewise for the R.k_sel = kc delivered triplets (nmf/nmf_init.hpp:71-79),
    // one launch a side and one download of len x k values a side.  Rows kc .. k - 1 are the reference's fill (:82-90): one
    // sequential SplitMix64 stream, the (k - kc) x m block of W column by column (rng.hpp:195-201), then the block of H.
    void nmf_start(Result& R, const T* Q, const T* Pm, int ja, int nbd, const std::vector<T>& wu, const std::vector<T>& wv,
                   const std::vector<double>& sig) {
        const int K = o.k, kc = R.k_sel;
        std::vector<T> hu((size_t)m * K, T(0)), hv((size_t)n * K, T(0));
        if (kc > 0) {
            std::vector<T> sq(kc);
            for (int c = 0; c < kc; ++c) sq[c] = std::sqrt((T)sig[c]);
            DevBuf dwu, dwv, dsq, ou, ov;
            upload_vec(wu, dwu);
            upload_vec(wv, dwv);
            upload_vec(sq, dsq);
            grow<T>(ou, hu.size()); grow<T>(ov, hv.size());
            HIPCHK(hipMemsetAsync(ou.p, 0, hu.size() * sizeof(T), s));
            HIPCHK(hipMemsetAsync(ov.p, 0, hv.size() * sizeof(T), s));
            const int chunks = (kc + NS_CW - 1) / NS_CW;
            hipLaunchKernelGGL(nmf_start_kernel<T>, dim3((m + WG - 1) / WG, chunks), dim3(WG), 0, s, Q, (long)m, ja,
                               (const T*)dwu.as<T>(), kc, (const T*)dsq.as<T>(), K, ou.as<T>());
            hipLaunchKernelGGL(nmf_start_kernel<T>, dim3((n + WG - 1) / WG, chunks), dim3(WG), 0, s, Pm, (long)n, nbd,
                               (const T*)dwv.as<T>(), kc, (const T*)dsq.as<T>(), K, ov.as<T>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(hu.data(), ou.p, hu.size() * sizeof(T), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hv.data(), ov.p, hv.size() * sizeof(T), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        if (kc < K) {
            const size_t rows = (size_t)(K - kc);
            const uint32_t fs = o.init_seed == 0 ? 54321u : o.init_seed + 999u;        // wraps in uint32, as the reference's does
            const std::vector<T> f = splitmix<T>(fs == 0 ? 12345ull : (uint64_t)fs, 0, rows * ((size_t)m + n));    // rng.hpp:73-74
            size_t q = 0;
            for (int j = 0; j < m; ++j)
                for (size_t i = 0; i < rows; ++i) hu[(size_t)j * K + kc + i] = f[q++];
            for (int j = 0; j < n; ++j)
                for (size_t i = 0; i < rows; ++i) hv[(size_t)j * K + kc + i] = f[q++];
        }
        R.U.assign(hu.begin(), hu.end());
        R.V.assign(hv.begin(), hv.end());
    }
    void upload_vec(const std::vector<T>& h, DevBuf& b) {
        grow<T>(b, h.size());
        HIPCHK(hipMemcpyAsync(b.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }

    // -------------------------------------------------------------------------------------------------------- KSPR
    // krylov.hpp:303-796 for L1 / L2 / nonneg / upper bound, FACTOR convergence: a Lanczos seed (or the caller's V0), then passes of
    // W = proj(A V (V'V + ridge)^-1), V = proj(A' W (W'W + ridge)^-1), six launches a pass (kernels_svd_krylov.hip.h) and no host
    // synchronisation inside a group of kPoll passes; Phase 3 on the host.
    void kspr(Result& R) {
        std::vector<double> seed_v;
        const double* V0 = o.V0;
        int K = o.k;
        R.passes = 0; R.dw.clear();
        if (!V0) {                                              // Phase 1, krylov.hpp:311-335
            lanczos(R);
            K = R.k_sel;
            R.iters.clear();
            if (K == 0) return;
            seed_v = R.V;
            V0 = seed_v.data();
        }
        const int maxp = o.ks_iter > 0 ? o.ks_iter : std::max(10, 2 * (int)std::ceil(std::log2((double)K)) + 3);
        const int kp = K > 32 ? WAVE : (int)std::max(1.0, std::exp2(std::ceil(std::log2((double)K))));
        const int nhm = (m + KS_RB - 1) / KS_RB, nhn = (n + KS_RB - 1) / KS_RB, ngm = (m + KS_GR - 1) / KS_GR, ngn = (n + KS_GR - 1) / KS_GR;
        const T eps = std::numeric_limits<T>::epsilon(), eps100 = eps * T(100);
        const double tol = (double)(T)o.tol;
        DevBuf bW[2], bV, bd, bPm, bPn, bPG, bGi, bLi, bns, bcs, bdw, st;
        T* W[2] = {grow<T>(bW[0], (size_t)K * m), grow<T>(bW[1], (size_t)K * m)};
        T* V = grow<T>(bV, (size_t)K * n);
        T* d = grow<T>(bd, K);
        double* Pm = grow<double>(bPm, (size_t)nhm * K);
        double* Pn = grow<double>(bPn, (size_t)nhn * K);
        double* PG = grow<double>(bPG, (size_t)std::max(ngm, ngn) * ks_np(K));
        double* Gi = grow<double>(bGi, (size_t)K * K);
        double* Li = grow<double>(bLi, (size_t)K * K);
        double* ns = grow<double>(bns, K);
        double* cs = grow<double>(bcs, K);
        double* dw = grow<double>(bdw, (size_t)maxp);
        int* S = grow<int>(st, S_WORDS);
        const int init[S_WORDS] = {INT_MAX, 0, 0, 0, 0, 0, 0, 0};
        std::vector<T> vt((size_t)K * n);
        for (int c = 0; c < K; ++c)
            for (int j = 0; j < n; ++j) vt[(size_t)j * K + c] = (T)V0[(size_t)c * n + j];
        HIPCHK(hipMemcpyAsync(V, vt.data(), vt.size() * sizeof(T), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(S, init, sizeof(init), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dw, 0, (size_t)maxp * sizeof(double), s));
        const double ru = 1e-12 + o.L2_u, rv = 1e-12 + o.L2_v;
        auto small = [&](int nb, double ridge, int it, int side, int last) {
            hipLaunchKernelGGL(ks_small_kernel, dim3(1), dim3(WG), 0, s, (const double*)PG, nb, K, ridge, Gi, Li, ns, cs, dw, tol, (double)eps,
                               S, it, side, last);
        };
        auto finish = [&](int nb, T* X, long len, const double* Pp, int nbh, int raw, const T* wt, const T* Xold, const int* stp, int it) {
            auto* f = RSV_BY_WIDTH(ks_finish_kernel, K);
            hipLaunchKernelGGL(f, dim3(nb), dim3(WG), 0, s, X, len, K, Pp, nbh, eps100, raw, wt, Xold, d, PG, stp, it);
        };
        // the seed's Gram and column sums: only V of the seed is read (krylov.hpp:472-524 overwrite W and d)
        finish(ngn, V, (long)n, nullptr, 0, 0, nullptr, nullptr, nullptr, 0);
        small(ngn, ru, -1, 1, 0);
        for (int done = 0; done < maxp;) {
            const int P = std::min(kPoll, maxp - done);
            for (int q = 0; q < P; ++q) {
                const int it = done + q;
                T* Wn = W[it & 1];
                const T* Wo = it > 0 ? W[(it & 1) ^ 1] : nullptr;
                hipLaunchKernelGGL(ks_half_kernel<T>, dim3(nhm), dim3(WG), 0, s, (const int*)Tp.as<int>(), (const int*)Ti.as<int>(),
                                   (const T*)Tx.as<T>(), (long)m, (const T*)V, K, kp, (const double*)Gi, (const double*)ns,
                                   (const double*)cs, mup(), o.center ? 1 : 0, (T)o.L1_u, o.nonneg_u, (T)o.ub_u, Wn, Pm, (const int*)S, it);
                finish(ngm, Wn, (long)m, Pm, nhm, 1, mup(), Wo, S, it);
                small(ngm, rv, it, 0, 0);
                hipLaunchKernelGGL(ks_half_kernel<T>, dim3(nhn), dim3(WG), 0, s, (const int*)Ap.as<int>(), (const int*)Ai.as<int>(),
                                   (const T*)Ax.as<T>(), (long)n, (const T*)Wn, K, kp, (const double*)Gi, (const double*)ns,
                                   (const double*)cs, (const T*)nullptr, o.center ? 2 : 0, (T)o.L1_v, o.nonneg_v, (T)o.ub_v, V, Pn,
                                   (const int*)S, it);
                finish(ngn, V, (long)n, Pn, nhn, 1, nullptr, nullptr, S, it);
                small(ngn, ru, it, 1, it == maxp - 1);
            }
            HIPCHK(hipGetLastError());
            done += P;
            if (read<int>(S + S_STOP, 1)[0] <= done) break;
        }
        const std::vector<int> sh = read<int>(S, S_WORDS);
        if (sh[KS_ERR]) {
            const int code = sh[KS_ERR] - 1;
            throw std::runtime_error("KSPR: non-positive Cholesky pivot in pass " + std::to_string(code / 2 + 1) + ", " +
                                     (code % 2 ? "V" : "W") + "-update: the Gram matrix of the fixed factor is not positive definite");
        }
        R.passes = sh[S_ITERS];
        const std::vector<T> wh = read<T>(W[(R.passes - 1) & 1], (size_t)K * m), vh = read<T>(V, (size_t)K * n), dh = read<T>(d, K);
        const std::vector<double> dwh = read<double>(dw, (size_t)maxp);
        R.dw.assign(dwh.begin(), dwh.begin() + std::max(R.passes - 1, 0));
        // ---- Phase 3 (krylov.hpp:742-781)
        std::vector<double> Uc((size_t)m * K), Vc((size_t)n * K);
        const bool hard = o.nonneg_u || o.nonneg_v || o.L1_u > 0 || o.L1_v > 0 || o.ub_u > 0 || o.ub_v > 0;
        R.k_sel = K;
        if (hard) {                                             // the factors as they are, by d descending (ties by index)
            std::vector<int> ord(K);
            std::iota(ord.begin(), ord.end(), 0);
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return dh[x] > dh[y]; });
            R.d.resize(K);
            for (int c = 0; c < K; ++c) {
                R.d[c] = (double)dh[ord[c]];
                for (int i = 0; i < m; ++i) Uc[(size_t)c * m + i] = (double)wh[(size_t)i * K + ord[c]];
                for (int j = 0; j < n; ++j) Vc[(size_t)c * n + j] = (double)vh[(size_t)j * K + ord[c]];
            }
            R.U.swap(Uc); R.V.swap(Vc);
            return;
        }
        for (int c = 0; c < K; ++c) {                           // L2 only: QR of W diag(d) and of V, SVD of R_w R_v'
            for (int i = 0; i < m; ++i) Uc[(size_t)c * m + i] = (double)wh[(size_t)i * K + c] * (double)dh[c];
            for (int j = 0; j < n; ++j) Vc[(size_t)c * n + j] = (double)vh[(size_t)j * K + c];
        }
        std::vector<double> Rw, Rv, Sm((size_t)K * K, 0.0), Us, Vs;
        mgs2_qr(Uc, m, K, Rw);
        mgs2_qr(Vc, n, K, Rv);
        for (int b = 0; b < K; ++b)
            for (int a = 0; a < K; ++a) {
                double acc = 0;
                for (int l = 0; l < K; ++l) acc += Rw[(size_t)l * K + a] * Rv[(size_t)l * K + b];
                Sm[(size_t)b * K + a] = acc;
            }
        jacobi_svd(Sm, K, Us, R.d, Vs);
        R.U = times_small(Uc, m, K, Us);
        R.V = times_small(Vc, n, K, Vs);
    }

    // -------------------------------------------------------------------------------------------------------- randomized
    // svd/randomized.hpp:59-241: Y = A~ Omega, q times (Q = orth(Y), Z = orth(A~' Q), Y = A~ Z), Q = orth(Y), Bt = A~' Q, and the
    // SVD of Bt.  orth() is CholeskyQR2 (a thin QR with positive pivots is unique up to column signs, which cancel in U d V'), and
    // the small SVD is the eigenproblem of the l x l Gram Bt'Bt on the host in fp64: sigma = sqrt(lambda), U = Q Vb, V = Bt Vb /
    // sigma.  Singular values below sqrt(eps) d_1 are not resolved that way, which a top-k fit does not need.  Four launches per
    // orth(), one per product, and no host synchronisation before the final Gram.
    void randomized(Result& R) {
        const int K = o.k, mn = std::min(m, n);
        const int p = std::min(std::max(10, K / 5), mn - K), l = K + std::max(p, 0);
        const int q = o.max_iter <= 0 ? 3 : std::min(o.max_iter, 10);
        const int lp = l > 32 ? WAVE : (int)std::max(1.0, std::exp2(std::ceil(std::log2((double)l))));
        const int nbm = (m + RS_RB - 1) / RS_RB, nbn = (n + RS_RB - 1) / RS_RB, np = rs_np(l);
        const double thr = (double)l * (double)std::numeric_limits<T>::epsilon();
        DevBuf bY, bZ, bPm, bPn, bRi, bLi, bG;
        T* Y = grow<T>(bY, (size_t)l * m);
        T* Z = grow<T>(bZ, (size_t)l * n);
        double* Pm = grow<double>(bPm, (size_t)nbm * np);
        double* Pn = grow<double>(bPn, (size_t)nbn * np);
        double* Ri = grow<double>(bRi, (size_t)l * l);
        double* Li = grow<double>(bLi, (size_t)l * l);
        double* G = grow<double>(bG, (size_t)l * l);
        auto* f_omega = RSV_BY_WIDTH(rs_omega_kernel, l);
        auto* f_prod = RSV_BY_WIDTH(rs_prod_kernel, l);
        auto* f_apply = RSV_BY_WIDTH(rs_apply_kernel, l);
        auto forward = [&] {        // Y = A~ Z
            hipLaunchKernelGGL(f_prod, dim3(nbm), dim3(WG), 0, s, (const int*)Tp.as<int>(), (const int*)Ti.as<int>(), (const T*)Tx.as<T>(),
                               (long)m, (const T*)Z, l, lp, (const double*)Pn, nbn, mup(), o.center ? 1 : 0, Y, Pm);
        };
        auto backward = [&] {       // Z = A~' Y
            hipLaunchKernelGGL(f_prod, dim3(nbn), dim3(WG), 0, s, (const int*)Ap.as<int>(), (const int*)Ai.as<int>(), (const T*)Ax.as<T>(),
                               (long)n, (const T*)Y, l, lp, (const double*)Pm, nbm, (const T*)nullptr, o.center ? 2 : 0, Z, Pn);
        };
        // X <- its orthonormal factor, twice; the last apply leaves the column sums the next product's centering reads (weights wt)
        auto orth = [&](T* X, long len, int nb, double* P, const T* wt) {
            hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)P, nb, l, thr, Ri, Li, G, 0);
            hipLaunchKernelGGL(f_apply, dim3(nb), dim3(WG), 0, s, X, len, l, (const double*)Ri, (const T*)nullptr, 1, P);
            hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)P, nb, l, thr, Ri, Li, G, 0);
            hipLaunchKernelGGL(f_apply, dim3(nb), dim3(WG), 0, s, X, len, l, (const double*)Ri, wt, 0, P);
        };
        hipLaunchKernelGGL(f_omega, dim3(nbn), dim3(WG), 0, s, Z, (long)n, l, (unsigned long long)(o.seed == 0 ? 42ull : (uint64_t)o.seed), Pn);
        forward();
        for (int it = 0; it < q; ++it) {
            orth(Y, (long)m, nbm, Pm, mup());
            backward();
            orth(Z, (long)n, nbn, Pn, (const T*)nullptr);
            forward();
        }
        orth(Y, (long)m, nbm, Pm, mup());
        backward();                                             // Bt, not orthonormalised
        hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)Pn, nbn, l, thr, Ri, Li, G, 1);
        HIPCHK(hipGetLastError());
        const std::vector<double> Gh = read<double>(G, (size_t)l * l);
        std::vector<double> Us, lam, Vb;
        jacobi_svd(Gh, l, Us, lam, Vb);                         // G is symmetric positive semidefinite: its SVD is its eigensystem
        const int kc = std::min(K, l);
        R.iters.assign(1, q);
        R.k_sel = kc;
        R.d.resize(kc);
        std::vector<double> wu((size_t)l * kc), wv((size_t)l * kc);
        for (int c = 0; c < kc; ++c) {
            const double sg = std::sqrt(std::max(lam[c], 0.0));
            R.d[c] = sg;
            for (int b = 0; b < l; ++b) {
                wu[(size_t)b * kc + c] = Vb[(size_t)c * l + b];
                wv[(size_t)b * kc + c] = sg > 0 ? Vb[(size_t)c * l + b] / sg : 0.0;
            }
        }
        DevBuf dwu, dwv, ou, ov;
        const double* Wu = upload<double>(dwu, wu.data(), wu.size(), s);
        const double* Wv = upload<double>(dwv, wv.data(), wv.size(), s);
        grow<T>(ou, (size_t)m * kc); grow<T>(ov, (size_t)n * kc);
        hipLaunchKernelGGL(rs_rotate_kernel<T>, dim3(wblk(m)), dim3(WG), 0, s, (const T*)Y, (long)m, l, Wu, kc, ou.as<T>());
        hipLaunchKernelGGL(rs_rotate_kernel<T>, dim3(wblk(n)), dim3(WG), 0, s, (const T*)Z, (long)n, l, Wv, kc, ov.as<T>());
        HIPCHK(hipGetLastError());
        R.U.resize((size_t)m * kc);
        R.V.resize((size_t)n * kc);
        download_cast<T>(g.c, ou, (size_t)m * kc, R.U.data(), s);
        download_cast<T>(g.c, ov, (size_t)n * kc, R.V.data(), s);
    }

    void run(Result& R) {
        R.row_means = mu_h;
        double f = 0;
        if (o.dense) for (size_t e = 0; e < (size_t)m * n; ++e) f += o.dense[e] * o.dense[e];
        else for (int64_t e = 0; e < o.nnz; ++e) f += o.x[e] * o.x[e];
        if (o.center) {
            double q = 0;
            for (double v : mu_h) q += v * v;
            f -= (double)n * q;
        }
        R.frob = f;
        R.n_test = (int)n_test;
        R.n_masked = n_masked;          // masked stored entries; every mask entry on a dense input (deflation.hpp:452-487)
        if (o.method == Method::randomized) randomized(R);
        else if (o.method == Method::kspr) kspr(R);
        else if (o.method == Method::deflation) deflation(R);
        else lanczos(R);
    }
};

// ------------------------------------------------------------------------------------------------------------ boundary
// Every check of an entry runs before any device work, and nothing is written on a refusal (status -1, the reason in
// rcppml_gpu_last_error).  A family's checks run in this order: null pointers, precision, the shape, the k_max range (load_checked
// / load_shared), then the family's own limit and its remaining checks (its make_*_opts), then the matrix (attach_csc /
// attach_dense).
struct Shared {   // the pointers every entry shares
    int* k_max; int *center, *seed; double *L1_u, *L1_v, *L2_u, *L2_v; int *nonneg_u, *nonneg_v; double *ub_u, *ub_v;
    double *U, *d, *V; int* out_k_selected; double *out_frobenius_norm_sq, *out_row_means, *out_wall_time_ms;
};
#define RCPPML_SVD_SHARED                                                                                                         \
    Shared{k_max, center, seed, L1_u, L1_v, L2_u, L2_v, nonneg_u, nonneg_v, ub_u, ub_v, U, d, V, out_k_selected,                  \
           out_frobenius_norm_sq, out_row_means, out_wall_time_ms}

// The shared fields of Opts.  The four reference entries call this as it is: they stay R-shaped, without a null check.
Opts load_shared(const Shared& a, int m, int n) {
    Opts o;
    o.m = m; o.n = n; o.k = *a.k_max;
    o.center = *a.center != 0; o.seed = (unsigned)(uint32_t)*a.seed;
    o.L1_u = *a.L1_u; o.L1_v = *a.L1_v; o.L2_u = *a.L2_u; o.L2_v = *a.L2_v; o.ub_u = *a.ub_u; o.ub_v = *a.ub_v;
    o.nonneg_u = *a.nonneg_u != 0; o.nonneg_v = *a.nonneg_v != 0;
    if (m < 1 || n < 1) throw std::invalid_argument("the matrix must have at least one row and one column");
    if (o.k < 1 || o.k > std::min(m, n)) throw std::invalid_argument("k_max must be in [1, min(m, n)]");
    return o;
}
// The build-defined entries: the null check (own_null: one of the family's own pointers is null) and the precision come first.
Opts load_checked(const Shared& a, const int* m, const int* n, const int* precision, bool own_null) {
    if (own_null || !m || !n || !precision || !a.k_max || !a.center || !a.seed || !a.L1_u || !a.L1_v || !a.L2_u || !a.L2_v ||
        !a.nonneg_u || !a.nonneg_v || !a.ub_u || !a.ub_v || !a.U || !a.d || !a.V || !a.out_k_selected || !a.out_frobenius_norm_sq ||
        !a.out_row_means || !a.out_wall_time_ms)
        throw std::invalid_argument("null pointer");
    if (*precision != RCPPML_F32 && *precision != RCPPML_F64)
        throw std::invalid_argument("precision must be RCPPML_F32 or RCPPML_F64");
    return load_shared(a, *m, *n);
}

void attach_csc(Opts& o, const int* col_ptr, const int* row_idx, const double* values, int64_t nnz) {
    o.nnz = nnz; o.p = col_ptr; o.i = row_idx; o.x = values;
    check_csc_lenient(o.p, o.i, o.x, o.m, o.n, o.nnz);
}
void attach_dense(Opts& o, const double* A) {
    if (!A) throw std::invalid_argument("null matrix");
    o.nnz = (int64_t)o.m * o.n; o.dense = A;
}
// An attached dense matrix enumerated as a full CSC too, as the reference's bridge does for krylov: what the block methods read.
struct FullCsc {
    std::vector<int> p, i;
    void attach(Opts& o) {
        if (o.nnz >= INT_MAX) throw std::invalid_argument("nnz out of range");
        p.resize((size_t)o.n + 1); i.resize((size_t)o.nnz);
        for (int j = 0; j <= o.n; ++j) p[j] = (int)((int64_t)j * o.m);
        for (int64_t e = 0; e < o.nnz; ++e) i[e] = (int)(e % o.m);
        o.p = p.data(); o.i = i.data(); o.x = o.dense;
    }
};

struct Fit { Result R; double ms; };
Fit timed_run(const Opts& o, bool f32) {
    Fit f;
    const auto t0 = std::chrono::steady_clock::now();
    if (f32) { Engine<float> E(o); E.run(f.R); }
    else { Engine<double> E(o); E.run(f.R); }
    f.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return f;
}
// The build-defined entries: the device and its free memory (need: a family's *_bytes estimate) are checked before the clock
// starts.
Fit fit(const Opts& o, int precision, size_t (*need)(const Opts&, size_t)) {
    const bool f32 = precision == RCPPML_F32;
    device_ready(need(o, f32 ? sizeof(float) : sizeof(double)), "the SVD");
    return timed_run(o, f32);
}

void write_shared(const Shared& a, const Opts& o, const Fit& f) {
    std::copy(f.R.U.begin(), f.R.U.end(), a.U);           // U: m x k_max, the first k_selected columns written
    std::copy(f.R.V.begin(), f.R.V.end(), a.V);
    std::copy(f.R.d.begin(), f.R.d.end(), a.d);
    *a.out_k_selected = f.R.k_sel;
    *a.out_frobenius_norm_sq = f.R.frob;
    if (o.center) std::copy(f.R.row_means.begin(), f.R.row_means.end(), a.out_row_means);
    *a.out_wall_time_ms = f.ms;
}

// ------------------------------------------------------------------------------------------------------------ reference entries
struct Raw {   // what only the four reference entries take (and read)
    double* tol; int* max_iter; double *L21_u, *L21_v, *angular_u, *angular_v;
    double* test_fraction; int* algorithm;
    int *graph_u_nnz; double* graph_u_lambda; int* graph_v_nnz; double* graph_v_lambda; int* obs_mask_nnz;
    int* out_iters_per_factor; double* robust_delta;
};

Opts make_opts(const Shared& s, const Raw& a, int m, int n) {
    Opts o = load_shared(s, m, n);
    o.tol = *a.tol; o.max_iter = *a.max_iter;
    const int algorithm = a.algorithm ? *a.algorithm : 0;
    if (o.k + 2 > NPMAX) throw std::invalid_argument("k_max above " + std::to_string(NPMAX - 2) + " is not supported");
    if (algorithm < 0 || algorithm > 4) throw std::invalid_argument("algorithm must be 0 (deflation) .. 4 (krylov)");
    o.method = algorithm == 0 ? Method::deflation : Method::lanczos;
    if (*a.test_fraction > 0) throw std::invalid_argument("test_fraction > 0 (cross-validation / auto-rank) is not supported on the GPU");
    if (a.obs_mask_nnz && *a.obs_mask_nnz > 0) throw std::invalid_argument("obs_mask is not supported on the GPU");
    if ((a.graph_u_nnz && *a.graph_u_nnz > 0 && *a.graph_u_lambda > 0) || (a.graph_v_nnz && *a.graph_v_nnz > 0 && *a.graph_v_lambda > 0))
        throw std::invalid_argument("graph regularization is not supported on the GPU");
    if ((a.L21_u && *a.L21_u != 0) || (a.L21_v && *a.L21_v != 0)) throw std::invalid_argument("L21 is not supported on the GPU");
    if ((a.angular_u && *a.angular_u != 0) || (a.angular_v && *a.angular_v != 0))
        throw std::invalid_argument("angular is not supported on the GPU");
    if (a.robust_delta && *a.robust_delta > 0) throw std::invalid_argument("robust SVD (robust_delta > 0) is not supported on the GPU");
    if (o.method != Method::deflation && has_constraints(o))
        throw std::invalid_argument("element constraints (L1 / L2 / nonneg / upper bound) need algorithm 0 (deflation) on the GPU");
    if (o.method == Method::deflation && o.max_iter < 1) throw std::invalid_argument("deflation needs max_iter >= 1");
    if (!(o.tol >= 0)) throw std::invalid_argument("tol must be non-negative");
    return o;
}

// the reference entries make no device_ready() call
void run_entry(const Shared& s, const Raw& a, const Opts& o, bool f32) {
    const Fit f = timed_run(o, f32);
    write_shared(s, o, f);
    for (int c = 0; c < (int)f.R.iters.size() && c < o.k; ++c) a.out_iters_per_factor[c] = f.R.iters[c];
}
void svd_sparse(bool f32, const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz, const Shared& s,
                const Raw& a, int* out_status) {
    entry_guard(out_status, [&] {
        Opts o = make_opts(s, a, *m, *n);
        attach_csc(o, col_ptr, row_idx, values, *nnz);
        run_entry(s, a, o, f32);
    });
}
void svd_dense(bool f32, const double* A, int* m, int* n, const Shared& s, const Raw& a, int* out_status) {
    entry_guard(out_status, [&] {
        Opts o = make_opts(s, a, *m, *n);
        attach_dense(o, A);
        run_entry(s, a, o, f32);
    });
}
}  // namespace

#define RCPPML_SVD_PARAMS                                                                                                         \
    int *k_max, double *U, double *d, double *V, double *tol, int *max_iter, int *center, int *verbose, int *seed, int *threads,     \
        double *L1_u, double *L1_v, double *L2_u, double *L2_v, int *nonneg_u, int *nonneg_v, double *ub_u, double *ub_v,          \
        double *L21_u, double *L21_v, double *angular_u, double *angular_v, double *test_fraction, int *cv_seed, int *patience,     \
        int *mask_zeros, int *algorithm, const int *graph_u_p, const int *graph_u_i, const double *graph_u_x, int *graph_u_dim,     \
        int *graph_u_nnz, double *graph_u_lambda_val, const int *graph_v_p, const int *graph_v_i, const double *graph_v_x,          \
        int *graph_v_dim, int *graph_v_nnz, double *graph_v_lambda_val, const int *obs_mask_p, const int *obs_mask_i,               \
        const double *obs_mask_x, int *obs_mask_rows, int *obs_mask_cols, int *obs_mask_nnz, int *out_k_selected,                   \
        double *out_wall_time_ms, double *out_test_loss, int *out_iters_per_factor, double *out_frobenius_norm_sq,                  \
        double *out_row_means, double *robust_delta, int *irls_max_iter, double *irls_tol, int *out_status
#define RCPPML_SVD_RAW                                                                                                            \
    Raw{tol, max_iter, L21_u, L21_v, angular_u, angular_v, test_fraction, algorithm, graph_u_nnz, graph_u_lambda_val, graph_v_nnz, \
        graph_v_lambda_val, obs_mask_nnz, out_iters_per_factor, robust_delta}

extern "C" void rcppml_gpu_svd_pca_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                          RCPPML_SVD_PARAMS) {
    svd_sparse(false, col_ptr, row_idx, values, m, n, nnz, RCPPML_SVD_SHARED, RCPPML_SVD_RAW, out_status);
}
extern "C" void rcppml_gpu_svd_pca_float(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                         RCPPML_SVD_PARAMS) {
    svd_sparse(true, col_ptr, row_idx, values, m, n, nnz, RCPPML_SVD_SHARED, RCPPML_SVD_RAW, out_status);
}
extern "C" void rcppml_gpu_svd_pca_dense_double(const double* A_data, int* m, int* n, RCPPML_SVD_PARAMS) {
    svd_dense(false, A_data, m, n, RCPPML_SVD_SHARED, RCPPML_SVD_RAW, out_status);
}
extern "C" void rcppml_gpu_svd_pca_dense_float(const double* A_data, int* m, int* n, RCPPML_SVD_PARAMS) {
    svd_dense(true, A_data, m, n, RCPPML_SVD_SHARED, RCPPML_SVD_RAW, out_status);
}

// ------------------------------------------------------------------------------------------------------------ cv and reg entries
// Build-defined.  cv: cross-validated / auto-rank and obs-masked deflation (the four entries above refuse both).  reg: the cv
// entries plus L21, angular and a graph per side (refused above too); with every new term off it is the cv entry, launch for
// launch.
namespace {
struct CvRaw {
    double* tol; int* max_iter; double* test_fraction; int *cv_seed, *patience, *mask_zeros;
    const int *obs_mask_p, *obs_mask_i; int *obs_mask_rows, *obs_mask_cols, *obs_mask_nnz;
    int* out_k_computed; double* out_test_loss; int *out_n_test, *out_n_masked, *out_iters_per_factor;
};

Opts make_cv_opts(const Shared& s, const CvRaw& a, const int* m, const int* n, const int* precision) {
    const bool own_null = !a.tol || !a.max_iter || !a.test_fraction || !a.cv_seed || !a.patience || !a.mask_zeros ||
                          !a.out_k_computed || !a.out_test_loss || !a.out_n_test || !a.out_n_masked || !a.out_iters_per_factor;
    Opts o = load_checked(s, m, n, precision, own_null);
    o.tol = *a.tol; o.max_iter = *a.max_iter;
    o.test_fraction = *a.test_fraction; o.patience = *a.patience; o.mask_zeros = *a.mask_zeros != 0;
    // core/svd_config.hpp:149-151
    const uint32_t cs = (uint32_t)*a.cv_seed;
    o.cv_seed = cs != 0 ? cs : (o.seed != 0 ? (uint32_t)(o.seed ^ 0xBEEFu) : 42u);
    if (o.k + 2 > NPMAX) throw std::invalid_argument("k_max above " + std::to_string(NPMAX - 2) + " is not supported");
    if (o.max_iter < 1) throw std::invalid_argument("deflation needs max_iter >= 1");
    if (o.patience < 1) throw std::invalid_argument("patience must be >= 1");
    if (!(o.test_fraction >= 0 && o.test_fraction < 1)) throw std::invalid_argument("test_fraction must be in [0, 1)");
    if (!(o.tol >= 0)) throw std::invalid_argument("tol must be non-negative");
    if (a.obs_mask_p) {
        if (!a.obs_mask_rows || !a.obs_mask_cols || !a.obs_mask_nnz) throw std::invalid_argument("null pointer");
        if (*a.obs_mask_rows != o.m || *a.obs_mask_cols != o.n) throw std::invalid_argument("obs_mask dimensions must match the matrix");
        o.mnnz = *a.obs_mask_nnz;
        if (o.mnnz < 0 || (o.mnnz > 0 && !a.obs_mask_i)) throw std::invalid_argument("null obs_mask array");
        check_csc_strict(a.obs_mask_p, a.obs_mask_i, o.m, o.n, o.mnnz);
        o.mp = a.obs_mask_p; o.mi = a.obs_mask_i;
    }
    return o;
}

// device bytes of a fit, generously: A, its transpose or training copy, the fp32 staging copy, twice the expected test entries,
// the factors and the partial buffers
size_t cv_bytes(const Opts& o, size_t ts) {
    const size_t len = o.dense ? (size_t)o.m * o.n : (size_t)o.nnz;
    size_t b = len * (o.dense ? 2 * ts : 2 * (sizeof(int) + ts) + ts) + len * sizeof(double);
    b += (size_t)(std::min(1.0, 2 * o.test_fraction) * (double)len) * (2 * sizeof(int) + ts);
    b += ((size_t)o.m + o.n) * ((size_t)o.k + 8) * ts + ((size_t)nblk(o.m) + nblk(o.n)) * ((size_t)o.k + 4) * ts;
    b += ((size_t)o.n + 1) * 3 * sizeof(int) + (size_t)o.mnnz * sizeof(int);
    return b;
}

void write_cv(const Shared& s, const CvRaw& a, const Opts& o, const Fit& f) {
    write_shared(s, o, f);
    std::copy(f.R.iters.begin(), f.R.iters.end(), a.out_iters_per_factor);
    std::copy(f.R.test_loss.begin(), f.R.test_loss.end(), a.out_test_loss);
    *a.out_k_computed = f.R.k_computed;
    *a.out_n_test = f.R.n_test;
    *a.out_n_masked = (int)f.R.n_masked;
}

struct RegRaw {
    double *L21_u, *L21_v, *angular_u, *angular_v;
    const int *graph_u_p, *graph_u_i; const double* graph_u_x; int *graph_u_dim, *graph_u_nnz; double* graph_u_lambda;
    const int *graph_v_p, *graph_v_i; const double* graph_v_x; int *graph_v_dim, *graph_v_nnz; double* graph_v_lambda;
};

Opts::Graph make_graph(const int* p, const int* i, const double* x, const int* dim, const int* nnz, const double* lambda, int want,
                       const char* name) {
    Opts::Graph gr;
    if (!p) return gr;
    if (!lambda) throw std::invalid_argument("null pointer");
    if (!(*lambda >= 0) || !std::isfinite(*lambda)) throw std::invalid_argument(std::string(name) + " lambda must be non-negative and finite");
    if (!(*lambda > 0)) return gr;
    if (!dim || !nnz) throw std::invalid_argument("null pointer");
    if (*dim != want)
        throw std::invalid_argument(std::string(name) + " must be " + std::to_string(want) + " x " + std::to_string(want) + " (dim " +
                                    std::to_string(*dim) + ")");
    try {
        check_csc_lenient(p, i, x, want, want, *nnz);
    } catch (const std::invalid_argument& e) {
        throw std::invalid_argument("malformed " + std::string(name) + " CSC: " + e.what());
    }
    all_finite(x, (size_t)*nnz, name);
    gr.p = p; gr.i = i; gr.x = x; gr.dim = want; gr.nnz = *nnz; gr.lambda = *lambda;
    return gr;
}

// Unlike every other family's own checks, these run after the matrix is attached and checked: a bad CSC or a null matrix wins.
void add_reg_opts(Opts& o, const RegRaw& r) {
    if (!r.L21_u || !r.L21_v || !r.angular_u || !r.angular_v) throw std::invalid_argument("null pointer");
    o.L21_u = *r.L21_u; o.L21_v = *r.L21_v; o.ang_u = *r.angular_u; o.ang_v = *r.angular_v;
    if (!(o.L21_u >= 0 && o.L21_v >= 0) || !std::isfinite(o.L21_u + o.L21_v))
        throw std::invalid_argument("L21 penalties must be non-negative and finite");
    if (!(o.ang_u >= 0 && o.ang_v >= 0) || !std::isfinite(o.ang_u + o.ang_v))
        throw std::invalid_argument("angular penalties must be non-negative and finite");
    o.gu = make_graph(r.graph_u_p, r.graph_u_i, r.graph_u_x, r.graph_u_dim, r.graph_u_nnz, r.graph_u_lambda, o.m, "graph_u");
    o.gv = make_graph(r.graph_v_p, r.graph_v_i, r.graph_v_x, r.graph_v_dim, r.graph_v_nnz, r.graph_v_lambda, o.n, "graph_v");
}

// cv_bytes plus the graphs (CSC, rows, fp64 staging), the chain's two partial buffers and L x
size_t reg_bytes(const Opts& o, size_t ts) {
    size_t b = cv_bytes(o, ts);
    for (const Opts::Graph* gr : {&o.gu, &o.gv})
        if (gr->on()) b += (size_t)gr->nnz * (2 * (sizeof(int) + ts) + sizeof(double)) + 2 * ((size_t)gr->dim + 1) * sizeof(int);
    b += 2 * (size_t)std::max(nblk(o.m), nblk(o.n)) * ((size_t)o.k + 2) * ts + (size_t)std::max(o.m, o.n) * ts;
    return b;
}
}  // namespace

#define RCPPML_SVD_CV_PARAMS                                                                                                      \
    int *precision, int *k_max, double *tol, int *max_iter, int *center, int *seed, double *L1_u, double *L1_v, double *L2_u,       \
        double *L2_v, int *nonneg_u, int *nonneg_v, double *ub_u, double *ub_v, double *test_fraction, int *cv_seed, int *patience, \
        int *mask_zeros, const int *obs_mask_p, const int *obs_mask_i, int *obs_mask_rows, int *obs_mask_cols, int *obs_mask_nnz,   \
        double *U, double *d, double *V, int *out_k_selected, int *out_k_computed, double *out_test_loss, int *out_n_test,          \
        int *out_n_masked, int *out_iters_per_factor, double *out_frobenius_norm_sq, double *out_row_means,                         \
        double *out_wall_time_ms, int *out_status
#define RCPPML_SVD_CV_RAW                                                                                                         \
    CvRaw{tol, max_iter, test_fraction, cv_seed, patience, mask_zeros, obs_mask_p, obs_mask_i, obs_mask_rows, obs_mask_cols,      \
          obs_mask_nnz, out_k_computed, out_test_loss, out_n_test, out_n_masked, out_iters_per_factor}

extern "C" void rcppml_gpu_svd_cv_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                     RCPPML_SVD_CV_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const CvRaw a = RCPPML_SVD_CV_RAW;
        Opts o = make_cv_opts(s, a, m, n, precision);
        if (!nnz) throw std::invalid_argument("null pointer");
        attach_csc(o, col_ptr, row_idx, values, *nnz);
        write_cv(s, a, o, fit(o, *precision, cv_bytes));
    });
}
extern "C" void rcppml_gpu_svd_cv_dense_ex(const double* A_data, int* m, int* n, RCPPML_SVD_CV_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const CvRaw a = RCPPML_SVD_CV_RAW;
        Opts o = make_cv_opts(s, a, m, n, precision);
        attach_dense(o, A_data);
        write_cv(s, a, o, fit(o, *precision, cv_bytes));
    });
}

#define RCPPML_SVD_REG_PARAMS                                                                                                     \
    int *precision, int *k_max, double *tol, int *max_iter, int *center, int *seed, double *L1_u, double *L1_v, double *L2_u,       \
        double *L2_v, int *nonneg_u, int *nonneg_v, double *ub_u, double *ub_v, double *L21_u, double *L21_v, double *angular_u,    \
        double *angular_v, const int *graph_u_p, const int *graph_u_i, const double *graph_u_x, int *graph_u_dim, int *graph_u_nnz, \
        double *graph_u_lambda, const int *graph_v_p, const int *graph_v_i, const double *graph_v_x, int *graph_v_dim,              \
        int *graph_v_nnz, double *graph_v_lambda, double *test_fraction, int *cv_seed, int *patience, int *mask_zeros,              \
        const int *obs_mask_p, const int *obs_mask_i, int *obs_mask_rows, int *obs_mask_cols, int *obs_mask_nnz, double *U,         \
        double *d, double *V, int *out_k_selected, int *out_k_computed, double *out_test_loss, int *out_n_test, int *out_n_masked,  \
        int *out_iters_per_factor, double *out_frobenius_norm_sq, double *out_row_means, double *out_wall_time_ms, int *out_status
#define RCPPML_SVD_REG_RAW                                                                                                        \
    RegRaw{L21_u, L21_v, angular_u, angular_v, graph_u_p, graph_u_i, graph_u_x, graph_u_dim, graph_u_nnz, graph_u_lambda,         \
           graph_v_p, graph_v_i, graph_v_x, graph_v_dim, graph_v_nnz, graph_v_lambda}

extern "C" void rcppml_gpu_svd_reg_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                      RCPPML_SVD_REG_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const CvRaw a = RCPPML_SVD_CV_RAW;
        Opts o = make_cv_opts(s, a, m, n, precision);
        if (!nnz) throw std::invalid_argument("null pointer");
        attach_csc(o, col_ptr, row_idx, values, *nnz);
        add_reg_opts(o, RCPPML_SVD_REG_RAW);
        write_cv(s, a, o, fit(o, *precision, reg_bytes));
    });
}
extern "C" void rcppml_gpu_svd_reg_dense_ex(const double* A_data, int* m, int* n, RCPPML_SVD_REG_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const CvRaw a = RCPPML_SVD_CV_RAW;
        Opts o = make_cv_opts(s, a, m, n, precision);
        attach_dense(o, A_data);
        add_reg_opts(o, RCPPML_SVD_REG_RAW);
        write_cv(s, a, o, fit(o, *precision, reg_bytes));
    });
}

// ------------------------------------------------------------------------------------------------------------ krylov entries
// Build-defined: the constrained block SVD (KSPR), which the four reference entries refuse as "algorithm 1-4 with element
// constraints".
namespace {
struct KsRaw {
    double* tol; int* max_iter; const double* V0; int* out_passes; double* out_dw;
};

Opts make_ks_opts(const Shared& s, const KsRaw& a, const int* m, const int* n, const int* precision) {
    Opts o = load_checked(s, m, n, precision, !a.tol || !a.max_iter || !a.out_passes || !a.out_dw);
    o.tol = *a.tol; o.max_iter = 0; o.ks_iter = *a.max_iter;
    o.method = Method::kspr; o.V0 = a.V0;
    if (o.k > KS_KMAX) throw std::invalid_argument("k_max above " + std::to_string(KS_KMAX) + " is not supported by the krylov method");
    if (!(o.tol >= 0)) throw std::invalid_argument("tol must be non-negative");
    if (!(o.L1_u >= 0 && o.L1_v >= 0)) throw std::invalid_argument("L1 penalties must be non-negative");
    if (!(o.L2_u >= 0 && o.L2_v >= 0)) throw std::invalid_argument("L2 penalties must be non-negative");
    if (!(o.ub_u >= 0 && o.ub_v >= 0)) throw std::invalid_argument("upper bounds must be non-negative");
    if (!std::isfinite(o.L1_u + o.L1_v + o.L2_u + o.L2_v + o.ub_u + o.ub_v + o.tol))
        throw std::invalid_argument("a penalty, bound or tol is not finite");
    if (!has_constraints(o))
        throw std::invalid_argument("the krylov method without element constraints is Lanczos: call rcppml_gpu_svd_pca_* with algorithm 2");
    if (a.V0) all_finite(a.V0, (size_t)o.n * o.k, "V0");
    return o;
}

// device bytes of a fit, generously: the CSC and its transpose with the fp64 staging copy (a dense input also as it is), the
// Lanczos bases of the seed, the block factors and the partial records
size_t ks_bytes(const Opts& o, size_t ts) {
    const size_t len = (size_t)o.nnz, K = (size_t)o.k, mn = (size_t)std::min(o.m, o.n);
    size_t b = len * (2 * (sizeof(int) + ts) + sizeof(double)) + (o.dense ? len * ts : 0) + ((size_t)o.m + o.n + 2) * sizeof(int);
    if (!o.V0) b += ((size_t)o.m + o.n) * (std::min(mn, std::max(3 * K, K + 50)) + 8) * ts;
    b += (2 * (size_t)o.m + o.n) * K * ts;
    b += ((size_t)o.m / KS_RB + o.n / KS_RB + 2) * K * sizeof(double) + ((size_t)std::max(o.m, o.n) / KS_GR + 1) * ks_np(o.k) * sizeof(double);
    return b + 3 * K * K * sizeof(double);
}

void write_ks(const Shared& s, const KsRaw& a, const Opts& o, const Fit& f) {
    write_shared(s, o, f);
    std::copy(f.R.dw.begin(), f.R.dw.end(), a.out_dw);
    *a.out_passes = f.R.passes;
}
}  // namespace

#define RCPPML_SVD_KS_PARAMS                                                                                                      \
    int *precision, int *k_max, double *tol, int *max_iter, int *center, int *seed, double *L1_u, double *L1_v, double *L2_u,       \
        double *L2_v, int *nonneg_u, int *nonneg_v, double *ub_u, double *ub_v, const double *V0, double *U, double *d, double *V,  \
        int *out_k_selected, int *out_passes, double *out_dw, double *out_frobenius_norm_sq, double *out_row_means,                 \
        double *out_wall_time_ms, int *out_status
#define RCPPML_SVD_KS_RAW KsRaw{tol, max_iter, V0, out_passes, out_dw}

extern "C" void rcppml_gpu_svd_krylov_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                         RCPPML_SVD_KS_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const KsRaw a = RCPPML_SVD_KS_RAW;
        Opts o = make_ks_opts(s, a, m, n, precision);
        if (!nnz) throw std::invalid_argument("null pointer");
        attach_csc(o, col_ptr, row_idx, values, *nnz);
        write_ks(s, a, o, fit(o, *precision, ks_bytes));
    });
}
// the block passes read the dense matrix as a full CSC; the Lanczos seed runs the dense products
extern "C" void rcppml_gpu_svd_krylov_dense_ex(const double* A_data, int* m, int* n, RCPPML_SVD_KS_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const KsRaw a = RCPPML_SVD_KS_RAW;
        Opts o = make_ks_opts(s, a, m, n, precision);
        attach_dense(o, A_data);
        FullCsc full;
        full.attach(o);
        write_ks(s, a, o, fit(o, *precision, ks_bytes));
    });
}

// ------------------------------------------------------------------------------------------------------------ randomized entries
// Build-defined: the randomized block SVD (svd/randomized.hpp:59-241), which the four reference entries run as Lanczos under
// algorithm 3.
namespace {
struct RsRaw {
    int* max_iter; double *L21_u, *L21_v, *angular_u, *angular_v;
    const int* graph_u_p; double* graph_u_lambda; const int* graph_v_p; double* graph_v_lambda; double* test_fraction;
    const int* obs_mask_p; int* out_iters;
};

int rs_sketch(int m, int n, int k) {        // randomized.hpp:73-74
    const int p = std::min(std::max(10, k / 5), std::min(m, n) - k);
    return k + std::max(p, 0);
}

Opts make_rs_opts(const Shared& s, const RsRaw& a, const int* m, const int* n, const int* precision) {
    const bool own_null = !a.max_iter || !a.L21_u || !a.L21_v || !a.angular_u || !a.angular_v || !a.test_fraction || !a.out_iters;
    Opts o = load_checked(s, m, n, precision, own_null);
    o.tol = 0; o.max_iter = *a.max_iter;
    o.method = Method::randomized;
    const int l = rs_sketch(o.m, o.n, o.k);
    if (l > RS_LMAX)
        throw std::invalid_argument("the randomized method's sketch dimension l = k + oversampling = " + std::to_string(l) +
                                    " is above the limit of " + std::to_string(RS_LMAX));
    if (has_constraints(o))
        throw std::invalid_argument("the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)");
    if (*a.L21_u != 0 || *a.L21_v != 0) throw std::invalid_argument("the randomized method does not support L21");
    if (*a.angular_u != 0 || *a.angular_v != 0) throw std::invalid_argument("the randomized method does not support angular");
    if ((a.graph_u_p && a.graph_u_lambda && *a.graph_u_lambda > 0) || (a.graph_v_p && a.graph_v_lambda && *a.graph_v_lambda > 0))
        throw std::invalid_argument("the randomized method does not support graph regularization");
    if (*a.test_fraction > 0) throw std::invalid_argument("the randomized method does not support test_fraction > 0 (cross-validation / auto-rank)");
    if (a.obs_mask_p) throw std::invalid_argument("the randomized method does not support obs_mask");
    return o;
}

// device bytes of a fit, generously: the CSC and its transpose with the fp64 staging copy, the row means, the two l-wide blocks,
// the rotated outputs with their fp64 staging, the block records and the small matrices
size_t rs_bytes(const Opts& o, size_t ts) {
    const size_t len = (size_t)o.nnz, K = (size_t)o.k, l = (size_t)rs_sketch(o.m, o.n, o.k);
    size_t b = len * (2 * (sizeof(int) + ts) + sizeof(double)) + ((size_t)o.m + o.n + 2) * sizeof(int) + (size_t)o.m * (ts + sizeof(double));
    b += ((size_t)o.m + o.n) * (l * ts + K * (ts + sizeof(double)));
    b += ((size_t)o.m / RS_RB + o.n / RS_RB + 2) * rs_np((int)l) * sizeof(double);
    return b + (3 * l * l + 2 * l * K) * sizeof(double);
}

void write_rs(const Shared& s, const RsRaw& a, const Opts& o, const Fit& f) {
    write_shared(s, o, f);
    std::copy(f.R.iters.begin(), f.R.iters.end(), a.out_iters);       // one value: the power iterations run
}
}  // namespace

#define RCPPML_SVD_RS_PARAMS                                                                                                      \
    int *precision, int *k_max, int *max_iter, int *center, int *seed, double *L1_u, double *L1_v, double *L2_u, double *L2_v,      \
        int *nonneg_u, int *nonneg_v, double *ub_u, double *ub_v, double *L21_u, double *L21_v, double *angular_u,                  \
        double *angular_v, const int *graph_u_p, double *graph_u_lambda, const int *graph_v_p, double *graph_v_lambda,              \
        double *test_fraction, const int *obs_mask_p, double *U, double *d, double *V, int *out_k_selected,                         \
        int *out_iters_per_factor, double *out_frobenius_norm_sq, double *out_row_means, double *out_wall_time_ms, int *out_status
#define RCPPML_SVD_RS_RAW                                                                                                         \
    RsRaw{max_iter, L21_u, L21_v, angular_u, angular_v, graph_u_p, graph_u_lambda, graph_v_p, graph_v_lambda, test_fraction,      \
          obs_mask_p, out_iters_per_factor}

// the finite check of the matrix follows its other checks
extern "C" void rcppml_gpu_svd_randomized_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                             RCPPML_SVD_RS_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const RsRaw a = RCPPML_SVD_RS_RAW;
        Opts o = make_rs_opts(s, a, m, n, precision);
        if (!nnz) throw std::invalid_argument("null pointer");
        attach_csc(o, col_ptr, row_idx, values, *nnz);
        all_finite(o.x, (size_t)o.nnz, "the matrix");
        write_rs(s, a, o, fit(o, *precision, rs_bytes));
    });
}
extern "C" void rcppml_gpu_svd_randomized_dense_ex(const double* A_data, int* m, int* n, RCPPML_SVD_RS_PARAMS) {
    entry_guard(out_status, [&] {
        const Shared s = RCPPML_SVD_SHARED;
        const RsRaw a = RCPPML_SVD_RS_RAW;
        Opts o = make_rs_opts(s, a, m, n, precision);
        attach_dense(o, A_data);
        FullCsc full;
        full.attach(o);
        all_finite(o.x, (size_t)o.nnz, "the matrix");
        write_rs(s, a, o, fit(o, *precision, rs_bytes));
    });
}

// ------------------------------------------------------------------------------------------------------------ NMF-start entries
// Build-defined: the SVD-seeded start of an NMF fit (nmf/nmf_init.hpp:45-158 initialize_lanczos / initialize_irlba, which R's
// nmf(seed = "lanczos" | "irlba") reaches as init_mode 1 / 2; the plugin's NMF ABI has no slot for init_mode).  The Lanczos engine
// with the reference's fixed options -- tol 1e-10, max_iter 0, no centring, the start vector of *seed -- in its NMF-start output
// mode.  Mode 2 runs the same engine, as algorithm 1 (irlba) does on the rcppml_gpu_svd_pca_* entries.
namespace {
struct NiRaw { int *k, *seed, *mode; double *W_T, *H, *d; int *out_k_svd, *out_iters; double* out_wall_time_ms; };

// device bytes of a call, generously: the matrix with its fp64 staging copy (and the CSR of a CSC), the two Lanczos bases, the
// work vectors and partials, the two k-wide outputs
size_t ni_bytes(const Opts& o, size_t ts) {
    const size_t len = (size_t)o.nnz, steps = (size_t)lanczos_steps(o.m, o.n, o.k, 0) + 2, mn = (size_t)o.m + o.n;
    size_t b = len * ((o.dense ? 1 : 2) * (sizeof(int) + ts) + sizeof(double)) + (mn + 2) * sizeof(int);
    b += mn * steps * ts + 4 * ((size_t)std::max(nblk(o.m), nblk(o.n))) * steps * ts + 3 * mn * ts;
    return b + mn * (size_t)o.k * ts;
}

template <class Attach> void nmf_svd_init(const int* m, const int* n, const int* precision, const NiRaw& a, Attach attach) {
    if (!a.k || !a.seed || !a.mode || !a.W_T || !a.H || !a.d || !a.out_k_svd || !a.out_iters || !a.out_wall_time_ms)
        throw std::invalid_argument("null pointer");
    // the shared fields the start does not have: no centring, no element constraints, and two outputs nobody reads
    int zero_i = 0;
    double zero_d = 0, frob = 0, no_means = 0;
    const Shared s{a.k, &zero_i, a.seed, &zero_d, &zero_d, &zero_d, &zero_d, &zero_i, &zero_i, &zero_d, &zero_d,
                   a.W_T, a.d, a.H, a.out_k_svd, &frob, &no_means, a.out_wall_time_ms};
    Opts o = load_checked(s, m, n, precision, false);
    if (*a.mode != 1 && *a.mode != 2) throw std::invalid_argument("mode must be 1 (lanczos) or 2 (irlba)");
    o.tol = 1e-10; o.max_iter = 0;
    o.method = Method::lanczos;
    o.nmf_start = true; o.init_seed = (uint32_t)*a.seed;
    (void)lanczos_steps(o.m, o.n, o.k, o.max_iter);        // the engine's own step limit, before any device work
    attach(o);
    all_finite(o.dense ? o.dense : o.x, (size_t)o.nnz, "the matrix");
    const Fit f = fit(o, *precision, ni_bytes);
    write_shared(s, o, f);
    *a.out_iters = f.R.iters.empty() ? 0 : f.R.iters[0];
}
}  // namespace

#define RCPPML_NMF_INIT_PARAMS                                                                                                    \
    int *precision, int *k, int *seed, int *mode, double *W_T, double *H, double *d, int *out_k_svd, int *out_iters,               \
        double *out_wall_time_ms, int *out_status
#define RCPPML_NMF_INIT_RAW NiRaw{k, seed, mode, W_T, H, d, out_k_svd, out_iters, out_wall_time_ms}

extern "C" void rcppml_gpu_nmf_svd_init_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                           RCPPML_NMF_INIT_PARAMS) {
    entry_guard(out_status, [&] {
        nmf_svd_init(m, n, precision, RCPPML_NMF_INIT_RAW, [&](Opts& o) {
            if (!nnz) throw std::invalid_argument("null pointer");
            attach_csc(o, col_ptr, row_idx, values, *nnz);
        });
    });
}
extern "C" void rcppml_gpu_nmf_svd_init_dense_ex(const double* A_data, int* m, int* n, RCPPML_NMF_INIT_PARAMS) {
    entry_guard(out_status, [&] { nmf_svd_init(m, n, precision, RCPPML_NMF_INIT_RAW, [&](Opts& o) { attach_dense(o, A_data); }); });
}

// Build-defined, for tools/init_bench.py: the device time of nmf_start_kernel beside the ritz_kernel launch it replaces, on one
// side of a start (a len x ja basis of uniform draws, kc of k columns), each the median of *reps timed launches after a warm-up,
// between two events on the stream.  Nothing of a fit runs here.
namespace {
template <class T> void start_time(long len, int ja, int kc, int k, int reps, double* start_ms, double* ritz_ms) {
    CtxGuard g(env_device());
    hipStream_t s = g.s;
    const std::vector<T> hb = splitmix<T>(42, 0, (size_t)len * ja), hw = splitmix<T>(43, 0, (size_t)ja * kc), hs = splitmix<T>(44, 0, (size_t)kc);
    DevBuf dB, dW, dS, o1, o2;
    const T* B = upload<T>(dB, hb.data(), hb.size(), s);
    const T* W = upload<T>(dW, hw.data(), hw.size(), s);
    const T* sq = upload<T>(dS, hs.data(), hs.size(), s);
    T* out_start = zeros<T>(o1, (size_t)len * k, s);
    T* out_ritz = zeros<T>(o2, (size_t)len * kc, s);
    HIPCHK(hipStreamSynchronize(s));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    auto median = [&](bool start) {
        std::vector<double> ms;
        for (int r = 0; r <= reps; ++r) {              // run 0 is the warm-up
            HIPCHK(hipEventRecord(e0, s));
            if (start)
                hipLaunchKernelGGL(nmf_start_kernel<T>, dim3((unsigned)((len + WG - 1) / WG), (kc + NS_CW - 1) / NS_CW), dim3(WG), 0, s, B, len,
                                   ja, W, kc, sq, k, out_start);
            else
                hipLaunchKernelGGL(ritz_kernel<T>, dim3((unsigned)((len + WG - 1) / WG), kc), dim3(WG), 0, s, B, len, ja, W, kc, out_ritz);
            HIPCHK(hipEventRecord(e1, s));
            HIPCHK(hipEventSynchronize(e1));
            HIPCHK(hipGetLastError());
            float t = 0;
            HIPCHK(hipEventElapsedTime(&t, e0, e1));
            if (r > 0) ms.push_back(t);
        }
        std::sort(ms.begin(), ms.end());
        return ms[ms.size() / 2];
    };
    *start_ms = median(true);
    *ritz_ms = median(false);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
}
}  // namespace

extern "C" void rcppml_hip_nmf_start_time(int* precision, int* len, int* ja, int* kc, int* k, int* reps, double* out_start_ms,
                                          double* out_ritz_ms, int* out_status) {
    entry_guard(out_status, [&] {
        if (!precision || !len || !ja || !kc || !k || !reps || !out_start_ms || !out_ritz_ms) throw std::invalid_argument("null pointer");
        if (*precision != RCPPML_F32 && *precision != RCPPML_F64) throw std::invalid_argument("precision must be RCPPML_F32 or RCPPML_F64");
        if (*len < 1 || *ja < 1 || *ja >= NPMAX || *kc < 1 || *kc > *k || *k >= NPMAX || *reps < 1 || *reps > 1000)
            throw std::invalid_argument("len >= 1, 1 <= ja < 4096, 1 <= kc <= k < 4096 and 1 <= reps <= 1000 are required");
        const size_t ts = *precision == RCPPML_F32 ? sizeof(float) : sizeof(double);
        device_ready(((size_t)*len * ((size_t)*ja + *k + *kc) + (size_t)*ja * *kc + *kc) * ts, "the timing");
        double a = 0, b = 0;
        if (*precision == RCPPML_F32) start_time<float>(*len, *ja, *kc, *k, *reps, &a, &b);
        else start_time<double>(*len, *ja, *kc, *k, *reps, &a, &b);
        *out_start_ms = a; *out_ritz_ms = b;
    });
}
