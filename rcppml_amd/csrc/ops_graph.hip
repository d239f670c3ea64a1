// ops_graph.hip -- factor graphs: the reference's multi-layer fit (inst/include/FactorNet/graph/fit.hpp:264-375, fit_deep) on the
// device, fp64.  Build-defined entry: R has no hook for it.
//
// fit_deep is an outer ALS: after a warm-up fit per layer, every outer iteration runs ONE iteration of the plain MSE fit on every
// layer (max_iter = 1, tol = 0, sort_model = false, started from the layer's W), each on a dense effective input assembled from the
// upstream layers' H (fit.hpp:100-194), and then recomputes every layer's reconstruction loss.  Through the plugin boundary that is
// max_iter x layers separate fits, each with its upload, transpose, plan set-up and download.  Here the first layer's matrix, its
// transpose and the right-hand-side plans are built once, every layer's W, d, H live on the device for the whole call, and the
// layers run on the fit's own device-level ops (Gram, right-hand sides on the CSC / its transpose / a dense array, CD or Cholesky
// solve, scaling, the Gram-trick loss), as ops_refine's W-refit cycles do.  What is new is in kernels_graph.hip.h: the assembly of an
// effective input and the explicit loss of a dense one.
//
// One iteration of a layer (nmf/fit_cpu.hpp, the standard path the reference takes for the dense inputs fit_deep hands over --
// fit.hpp:277 densifies the first layer's data too):  G = W_T W_T^T + 1e-15 I (+ L2_H);  B = W_T X;  H = solve(G, B - L1_H), from zero
// in a fit's first iteration (warm_start = iter > 0, fit_cpu.hpp:630, :879) and from the residual-corrected previous H afterwards (CD
// only; the warm-up's later iterations);  upper bound;  H -> d;  the same for W on X^T.  A sparse first layer takes the same steps
// with the sparse right-hand sides: the same sums over the nonzeros only.
//
// Losses.  A dense effective input: the explicit sum of squares (graph_layer_loss_kernel).  A sparse first layer: the Gram trick
// ||A||^2 - 2 <W diag(d), A H^T> + <G_w diag-scaled, G_h> on the right-hand side the W update has just formed (no eps in either
// Gram).  The warm-up's convergence rule reads the fit's own Gram-trick loss (fit_cpu.hpp:1710-1753), and only when tol > 0.
#include "entry_common.hip.h"
#include "kernels_graph.hip.h"

#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace {
using namespace rcppml_plugin;
using namespace rgraph;

constexpr double kEps = 1e-15;          // nmf/fit_cpu.hpp:491, :715
constexpr int kMaxLayers = 64;
enum { SRC_INPUT = 0, SRC_LAYER = 1, SRC_CONCAT = 2, SRC_ADD = 3 };

void assemble_launch(hipStream_t s, const AssembleArgs& a, int64_t n, double* X) {
    const int c_total = a.kcols + a.p;
    if (n <= 0 || c_total <= 0) return;
    const dim3 grid((unsigned)((n + TILE - 1) / TILE), (unsigned)((c_total + TILE - 1) / TILE));
    hipLaunchKernelGGL(graph_assemble_kernel, grid, dim3(NT), 0, s, a, n, X);
    HIPCHK(hipGetLastError());
}

AssembleArgs assemble_args(int mode, int nb, const void* const* H, const int* k, const void* Z, int p) {
    if (mode != GRAPH_CONCAT && mode != GRAPH_ADD) throw std::invalid_argument("graph_assemble: mode must be 0 (concat) or 1 (add)");
    if (nb < 1 || nb > GRAPH_MAX_BRANCHES) throw std::invalid_argument("graph_assemble: 1 to 8 branches");
    if (p < 0 || (p > 0 && !Z)) throw std::invalid_argument("graph_assemble: a condition block needs Z and p >= 0");
    AssembleArgs a{};
    int off = 0;
    for (int b = 0; b < nb; ++b) {
        if (!H[b] || k[b] < 1) throw std::invalid_argument("graph_assemble: a branch needs a factor and a rank >= 1");
        if (mode == GRAPH_ADD && k[b] != k[0]) throw std::invalid_argument("graph_assemble: add needs equal branch ranks");
        a.H[b] = static_cast<const double*>(H[b]);
        a.kb[b] = k[b];
        a.off[b] = off;
        off += k[b];
    }
    a.nb = nb;
    a.mode = mode;
    a.kcols = mode == GRAPH_ADD ? k[0] : off;
    a.Z = p > 0 ? static_cast<const double*>(Z) : nullptr;
    a.p = p;
    return a;
}

void layer_loss_launch(rcppml_hip_ctx* c, const double* X, int64_t rows, int cols, const double* W_T, const double* d, const double* H,
                       int k, double scale, double* out) {
    if (k < 1 || k > GRAPH_MAX_K) throw std::invalid_argument("graph_layer_loss: k must be in [1, 128]");
    if (rows < 1 || cols < 1) throw std::invalid_argument("graph_layer_loss: rows and c must be >= 1");
    const int64_t nblk = (rows + LOSS_ROWS - 1) / LOSS_ROWS;
    if (nblk >= ((int64_t)1 << 31)) throw std::invalid_argument("graph_layer_loss: too many rows");
    double* partial = static_cast<double*>(c->scratch(WS_RED, (size_t)nblk * sizeof(double)));
    const size_t lds = loss_lds_bytes(k);
    static DynSmemOnce once;
    once.ensure(reinterpret_cast<const void*>(graph_layer_loss_kernel), lds, c->device);
    hipLaunchKernelGGL(graph_layer_loss_kernel, dim3((unsigned)nblk), dim3(NT), lds, c->stream, X, rows, cols, W_T, d, H, k, partial);
    hipLaunchKernelGGL(graph_loss_final_kernel, dim3(1), dim3(NT), 0, c->stream, partial, nblk, scale, out);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" int rcppml_hip_graph_assemble(rcppml_hip_ctx* c, int dtype, int mode, int n_branches, const void* const* H, const int* k,
                                         int64_t n, const void* Z, int p, void* X) {
    try {
        if (dtype != RCPPML_F64) throw std::invalid_argument("graph_assemble: fp64 only");
        if (!H || !k || !X) throw std::invalid_argument("graph_assemble: null argument");
        HIPCHK(hipSetDevice(c->device));
        assemble_launch(c->stream, assemble_args(mode, n_branches, H, k, Z, p), n, static_cast<double*>(X));
        return 0;
    }
    RCPPML_CATCH_RET
}

extern "C" int rcppml_hip_graph_layer_loss(rcppml_hip_ctx* c, int dtype, const void* X, int64_t rows, int cols, const void* W_T,
                                           const void* d, const void* H, int k, double scale, double* out) {
    try {
        if (dtype != RCPPML_F64) throw std::invalid_argument("graph_layer_loss: fp64 only");
        if (!X || !W_T || !d || !H || !out) throw std::invalid_argument("graph_layer_loss: null argument");
        HIPCHK(hipSetDevice(c->device));
        layer_loss_launch(c, static_cast<const double*>(X), rows, cols, static_cast<const double*>(W_T), static_cast<const double*>(d),
                          static_cast<const double*>(H), k, scale, out);
        return 0;
    }
    RCPPML_CATCH_RET
}

namespace {

// ------------------------------------------------------------------------------------------------------------------ the graph
struct Layer {
    int k = 0, kind = 0, p = 0;
    std::vector<int> br;
    int64_t rows = 0, cols = 0;
    size_t offW = 0, offd = 0, offH = 0, offZ = 0;      // element offsets into the packed W, d, H and cond_Z
    double L1w = 0, L1h = 0, L2w = 0, L2h = 0, ubw = 0, ubh = 0;
    int nnw = 1, nnh = 1;
    DevBuf W, d, H, Z, Bw;                                  // Bw: the raw right-hand side of the last W update (sparse input layers)
};

struct Plan {
    rcppml_rhs_plan* p = nullptr;
    ~Plan() { if (p) rcppml_hip_rhs_plan_destroy(p); }
};

// The first layer's data on the device: the CSC with its device-side transpose, or the dense array.  Built once per call.
struct InputMatrix {
    bool dense = false;
    int64_t m = 0, n = 0, nnz = 0;
    DevBuf Ap, Ai, Ax, Tp, Ti, Tx, tr;
    size_t bytes() const { return dense ? 8 * (size_t)(m * n) : 2 * ((size_t)(m + n + 2) * 4 + (size_t)nnz * 12); }
};

struct Engine {
    rcppml_hip_ctx* c;
    hipStream_t s;
    InputMatrix& A;
    std::vector<Layer>& L;
    std::vector<Plan> planA, planT;                          // per layer (input layers of a large sparse matrix only)
    int solver_mode, norm_type, cd_maxit;
    double cd_tol;
    DevBuf X, Bh, Bw, G, Gs, Gwt, sums, loss3, losses, total, trX;
    int ops = 0, launches = 0;                               // counted while `counting`
    bool counting = false;

    void op() { if (counting) ++ops; }

    const double* effective_input(int i) {
        Layer& l = L[(size_t)i];
        if (l.kind == SRC_INPUT) return A.dense ? A.Ax.as<double>() : nullptr;
        const void* hp[GRAPH_MAX_BRANCHES];
        int kb[GRAPH_MAX_BRANCHES];
        for (size_t b = 0; b < l.br.size(); ++b) {
            hp[b] = L[(size_t)l.br[b]].H.p;
            kb[b] = L[(size_t)l.br[b]].k;
        }
        assemble_launch(s, assemble_args(l.kind == SRC_ADD ? GRAPH_ADD : GRAPH_CONCAT, (int)l.br.size(), hp, kb, l.Z.p, l.p), l.rows,
                        X.as<double>());
        if (counting) ++launches;
        return X.as<double>();
    }
    // B (k x cols) = F (k x rows) X
    void rhs_cols(int i, const double* Xd, const void* F, void* B) {
        Layer& l = L[(size_t)i];
        op();
        if (Xd) OPCHK(rcppml_hip_rhs_dense(c, RCPPML_F64, Xd, l.rows, l.cols, 0, F, l.k, B));
        else if (planA[(size_t)i].p) OPCHK(rcppml_hip_rhs_planned(c, planA[(size_t)i].p, F, B));
        else OPCHK(rcppml_hip_rhs(c, RCPPML_F64, A.Ap.as<int>(), A.Ai.as<int>(), A.Ax.p, A.n, F, l.k, B));
    }
    // B (k x rows) = F (k x cols) X^T
    void rhs_rows(int i, const double* Xd, const void* F, void* B) {
        Layer& l = L[(size_t)i];
        op();
        if (Xd) OPCHK(rcppml_hip_rhs_dense(c, RCPPML_F64, Xd, l.rows, l.cols, 1, F, l.k, B));
        else if (planT[(size_t)i].p) OPCHK(rcppml_hip_rhs_planned(c, planT[(size_t)i].p, F, B));
        else OPCHK(rcppml_hip_rhs(c, RCPPML_F64, A.Tp.as<int>(), A.Ti.as<int>(), A.Tx.p, A.m, F, l.k, B));
    }
    void solve(const void* Gm, const void* B, void* Xo, int k, int64_t ncols, double l1, int nonneg, double ub, bool warm) {
        op();
        if (solver_mode == 0)
            OPCHK(rcppml_hip_solve_cd(c, RCPPML_F64, Gm, B, Xo, k, ncols, l1 > 0 ? l1 : 0.0, warm ? 1 : 0, warm ? 0 : 1, 0.0, 0.0, nonneg,
                                      cd_maxit, cd_tol, 0.0, ub, RCPPML_CD_AUTO, nullptr, nullptr));
        else
            OPCHK(rcppml_hip_solve_chol(c, RCPPML_F64, Gm, B, Xo, k, ncols, l1 > 0 ? l1 : 0.0, nonneg, ub));
    }
    // one iteration of layer i's fit on Xd (nullptr: the sparse input); `warm`: not the fit's first iteration
    // returns the buffer that holds the raw right-hand side of the W update
    void* iterate(int i, const double* Xd, bool warm) {
        Layer& l = L[(size_t)i];
        const int k = l.k;
        // H half-update (fit_cpu.hpp:486-645)
        op();
        OPCHK(rcppml_hip_gram(c, RCPPML_F64, l.W.p, k, l.rows, kEps, l.L2h, G.p));
        rhs_cols(i, Xd, l.W.p, Bh.p);
        solve(G.p, Bh.p, l.H.p, k, l.cols, l.L1h, l.nnh, l.ubh, warm);
        op();
        OPCHK(rcppml_hip_scale_order(c, RCPPML_F64, l.H.p, k, l.cols, norm_type, sums.p, l.d.p, nullptr, nullptr));
        // W half-update (:711-893); G_saved = gram(H) + eps before the features (:715-722)
        op();
        OPCHK(rcppml_hip_gram(c, RCPPML_F64, l.H.p, k, l.cols, kEps, 0.0, Gs.p));
        const void* Gw = Gs.p;
        if (l.L2w > 0) {
            op();
            OPCHK(rcppml_hip_gram(c, RCPPML_F64, l.H.p, k, l.cols, kEps, l.L2w, G.p));
            Gw = G.p;
        }
        void* bw = l.Bw.p ? l.Bw.p : Bw.p;
        rhs_rows(i, Xd, l.H.p, bw);
        solve(Gw, bw, l.W.p, k, l.rows, l.L1w, l.nnw, l.ubw, warm);
        op();
        OPCHK(rcppml_hip_scale_order(c, RCPPML_F64, l.W.p, k, l.rows, norm_type, sums.p, l.d.p, nullptr, nullptr));
        return bw;
    }
    double read_scalar(const double* dptr) {
        double v = 0;
        download(&v, dptr, 1, s);
        return v;
    }
    // the reference's warm-up fit of layer i: min(10, max_iter) iterations with the fit's own convergence rule (fit_cpu.hpp:1769-1807)
    void warm_up(int i, int iters, double tol) {
        Layer& l = L[(size_t)i];
        const double* Xd = effective_input(i);
        if (tol > 0) {
            if (Xd) OPCHK(rcppml_hip_sumsq(c, RCPPML_F64, Xd, l.rows * l.cols, trX.as<double>()));
            else OPCHK(rcppml_hip_sumsq(c, RCPPML_F64, A.Ax.p, A.nnz, trX.as<double>()));
        }
        double prev = std::numeric_limits<double>::max();
        int patience = 0;
        for (int it = 0; it < iters; ++it) {
            void* bw = iterate(i, Xd, it > 0);
            if (!(tol > 0)) continue;                            // rel < tol never holds: the loss is not needed
            OPCHK(rcppml_hip_gram_loss_mse(c, RCPPML_F64, l.W.p, l.k, l.rows, kEps, trX.as<double>(), l.d.p, bw, Gs.p, Gwt.p,
                                           loss3.as<double>()));
            const double loss = read_scalar(loss3.as<double>());
            bool conv = false;
            if (it > 0) conv = std::fabs(prev - loss) / (std::fabs(prev) + 1e-15) < tol;
            prev = loss;
            if (it > 0) {
                if (conv) { if (++patience >= 5) break; }
                else patience = 0;
            }
        }
    }
    // layer i's mean squared reconstruction error -> layer_loss[i] (fit.hpp:329-338)
    void layer_loss(int i) {
        Layer& l = L[(size_t)i];
        const double* Xd = effective_input(i);
        const double scale = 1.0 / ((double)l.rows * (double)l.cols);
        double* out = losses.as<double>() + i;
        if (Xd) {
            op();
            layer_loss_launch(c, Xd, l.rows, (int)l.cols, l.W.as<double>(), l.d.as<double>(), l.H.as<double>(), l.k, scale, out);
            return;
        }
        // sparse input: the Gram trick on the right-hand side H A^T of the layer's last W update (H has not changed since)
        op();
        OPCHK(rcppml_hip_gram(c, RCPPML_F64, l.H.p, l.k, l.cols, 0.0, 0.0, Gs.p));
        op();
        OPCHK(rcppml_hip_gram_loss_mse(c, RCPPML_F64, l.W.p, l.k, l.rows, 0.0, A.tr.as<double>(), l.d.p, l.Bw.p, Gs.p, Gwt.p,
                                       loss3.as<double>()));
        hipLaunchKernelGGL(graph_scale_scalar_kernel, dim3(1), dim3(64), 0, s, loss3.as<double>(), scale, out);
        HIPCHK(hipGetLastError());
        if (counting) ++launches;
    }
    double total_loss() {
        hipLaunchKernelGGL(graph_sum_scalars_kernel, dim3(1), dim3(64), 0, s, losses.as<double>(), (int)L.size(), total.as<double>());
        HIPCHK(hipGetLastError());
        if (counting) ++launches;
        return read_scalar(total.as<double>());
    }
};

template <class T> const T& need(const T* p, const char* what) {
    if (!p) throw std::invalid_argument(std::string("null ") + what);
    return *p;
}

}  // namespace

extern "C" void rcppml_gpu_factor_net_fit_ex(const int* col_ptr, const int* row_idx, const double* values, int* nnz, const double* dense,
                                             int* m, int* n, int* n_layers, const int* rank, const int* src_kind,
                                             const int* branch_ptr, const int* branch_idx, const int* cond_p, const double* cond_Z,
                                             const double* L1, const double* L2, const double* upper_bound, const int* nonneg,
                                             int* max_iter, double* tol, int* seed, int* solver_mode, int* norm_type, int* cd_maxit,
                                             double* cd_tol, int* start, double* W, double* d, double* H, double* out_layer_loss,
                                             int* out_iter, int* out_converged, double* out_loss, int* out_counts, int* out_status) {
    entry_guard(out_status, [&] {
        const int64_t M = need(m, "m"), N = need(n, "n");
        const int NL = need(n_layers, "n_layers");
        const int maxit = need(max_iter, "max_iter"), smode = need(solver_mode, "solver_mode"), ntype = need(norm_type, "norm_type");
        const int cdit = need(cd_maxit, "cd_maxit"), st = need(start, "start");
        const double tl = need(tol, "tol"), cdt = need(cd_tol, "cd_tol");
        const uint32_t seed_base = need(seed, "seed") ? (uint32_t)*seed : 42u;           // fit.hpp:273-274
        if (!rank || !src_kind || !branch_ptr || !cond_p || !L1 || !L2 || !upper_bound || !nonneg) throw std::invalid_argument("null graph array");
        if (!W || !d || !H || !out_layer_loss || !out_iter || !out_converged || !out_loss) throw std::invalid_argument("null output");
        if (M < 1 || N < 1) throw std::invalid_argument("m and n must be >= 1");
        if (NL < 1 || NL > kMaxLayers) throw std::invalid_argument("n_layers must be in [1, 64]");
        if (maxit < 1) throw std::invalid_argument("max_iter must be >= 1");
        if (smode != 0 && smode != 1) throw std::invalid_argument("solver_mode must be 0 (CD) or 1 (Cholesky)");
        if (ntype < 0 || ntype > 2) throw std::invalid_argument("norm_type must be 0 (L1), 1 (L2) or 2 (none)");
        if (cdit < 1) throw std::invalid_argument("cd_maxit must be >= 1");
        if (!(tl >= 0) || !(cdt >= 0)) throw std::invalid_argument("tol and cd_tol must be >= 0");
        if (st != 0 && st != 1) throw std::invalid_argument("start must be 0 or 1");

        // ---- the graph
        std::vector<Layer> layers((size_t)NL);
        size_t oW = 0, od = 0, oH = 0, oZ = 0;
        if (branch_ptr[0] != 0) throw std::invalid_argument("branch_ptr must start at 0");
        int64_t max_rows = 0, max_cols = 0, max_x = 0;
        for (int i = 0; i < NL; ++i) {
            Layer& l = layers[(size_t)i];
            l.k = rank[i]; l.kind = src_kind[i]; l.p = cond_p[i];
            if (l.k < 1 || l.k > GRAPH_MAX_K) throw std::invalid_argument("layer " + std::to_string(i) + ": the rank must be in [1, 128]");
            if (smode == 1 && l.k > 64)
                throw std::invalid_argument("layer " + std::to_string(i) + ": the Cholesky solver needs a rank <= 64 (the fp64 Cholesky solve)");
            if (l.kind < SRC_INPUT || l.kind > SRC_ADD) throw std::invalid_argument("src_kind must be 0 (input), 1 (layer), 2 (concat) or 3 (add)");
            const int b0 = branch_ptr[i], b1 = branch_ptr[i + 1];
            if (b1 < b0) throw std::invalid_argument("branch_ptr decreases");
            const int nb = b1 - b0;
            if (nb > 0 && !branch_idx) throw std::invalid_argument("null graph array");
            if ((l.kind == SRC_INPUT && nb != 0) || (l.kind == SRC_LAYER && nb != 1) ||
                (l.kind >= SRC_CONCAT && (nb < 2 || nb > GRAPH_MAX_BRANCHES)))
                throw std::invalid_argument("layer " + std::to_string(i) + ": input takes no branch, layer one, concat and add 2 to 8");
            if (l.p < 0 || (l.p > 0 && (l.kind == SRC_INPUT || !cond_Z)))
                throw std::invalid_argument("layer " + std::to_string(i) + ": a condition block needs an upstream layer, Z and p >= 0");
            if (l.kind == SRC_INPUT) { l.rows = M; l.cols = N; }
            else {
                int64_t ksum = 0;
                for (int q = b0; q < b1; ++q) {
                    const int b = branch_idx[q];
                    if (b < 0 || b >= i) throw std::invalid_argument("layer " + std::to_string(i) + ": a branch must be an earlier layer");
                    const Layer& u = layers[(size_t)b];
                    if (q == b0) l.rows = u.cols;
                    else if (u.cols != l.rows) throw std::invalid_argument("layer " + std::to_string(i) + ": the branches' H differ in their number of columns");
                    if (l.kind == SRC_ADD && u.k != layers[(size_t)branch_idx[b0]].k)
                        throw std::invalid_argument("layer " + std::to_string(i) + ": add needs equal branch ranks");
                    ksum += u.k;
                    l.br.push_back(b);
                }
                l.cols = (l.kind == SRC_ADD ? layers[(size_t)branch_idx[b0]].k : ksum) + l.p;
                max_x = std::max(max_x, l.rows * l.cols);
            }
            if (l.rows >= ((int64_t)1 << 31) || l.cols >= ((int64_t)1 << 31)) throw std::invalid_argument("a layer's input is too large");
            l.L1w = L1[2 * i]; l.L1h = L1[2 * i + 1]; l.L2w = L2[2 * i]; l.L2h = L2[2 * i + 1];
            l.ubw = upper_bound[2 * i]; l.ubh = upper_bound[2 * i + 1];
            l.nnw = nonneg[2 * i] != 0; l.nnh = nonneg[2 * i + 1] != 0;
            for (double v : {l.L1w, l.L1h, l.L2w, l.L2h, l.ubw, l.ubh})
                if (!std::isfinite(v) || v < 0) throw std::invalid_argument("L1, L2 and upper_bound must be finite and >= 0");
            l.offW = oW; l.offd = od; l.offH = oH; l.offZ = oZ;
            oW += (size_t)l.k * (size_t)l.rows; od += (size_t)l.k; oH += (size_t)l.k * (size_t)l.cols; oZ += (size_t)l.p * (size_t)l.rows;
            max_rows = std::max(max_rows, l.rows); max_cols = std::max(max_cols, l.cols);
        }
        if (oZ) all_finite(cond_Z, oZ, "Z");
        if (st == 1) { all_finite(W, oW, "W"); all_finite(d, od, "d"); all_finite(H, oH, "H"); }

        // ---- the first layer's data
        if (col_ptr && dense) throw std::invalid_argument("give the matrix either as a CSC or as a dense array, not both");
        if (!col_ptr && !dense) throw std::invalid_argument("give the matrix as a CSC or as a dense array");
        InputMatrix A;
        A.m = M; A.n = N; A.dense = dense != nullptr;
        if (col_ptr) {
            if (!nnz || *nnz < 0) throw std::invalid_argument("nnz must be >= 0");
            if (*nnz > 0 && (!row_idx || !values)) throw std::invalid_argument("null CSC array");
            A.nnz = *nnz;
            check_csc_strict(col_ptr, row_idx, M, N, A.nnz);
            all_finite(values, (size_t)A.nnz, "the matrix");
        } else {
            if (M * N >= ((int64_t)1 << 40)) throw std::invalid_argument("the dense matrix is too large");
            all_finite(dense, (size_t)(M * N), "the matrix");
        }

        // ---- memory guard: the matrix (a sparse one with its transpose), every layer's W, d, H, Z and a sparse input layer's Bw, the
        // work buffers (X, Bh, Bw, three Grams), and as much again as the matrix for the plans of a large sparse input
        size_t need_b = A.bytes() + 8 * (oW + od + oH + oZ) + 8 * ((size_t)max_x + (size_t)GRAPH_MAX_K * (size_t)(max_rows + max_cols)) +
                        8 * (size_t)(3 * GRAPH_MAX_K * GRAPH_MAX_K + 4 * GRAPH_MAX_K + kMaxLayers + 16) + (1u << 20);
        int n_input_layers = 0;
        for (const Layer& l : layers)
            if (l.kind == SRC_INPUT) { ++n_input_layers; if (!A.dense) need_b += 8 * (size_t)l.k * (size_t)M; }
        if (!A.dense && A.nnz >= (1 << 20)) need_b += (size_t)n_input_layers * A.bytes();
        device_ready(need_b, "the factor graph fit");

        CtxGuard g(env_device());
        rcppml_hip_ctx* c = g.c;
        hipStream_t s = g.s;
        if (A.dense) {
            upload(A.Ax, dense, (size_t)(M * N), s);
        } else {
            upload(A.Ap, col_ptr, (size_t)N + 1, s);
            upload(A.Ai, row_idx, (size_t)A.nnz, s);
            upload(A.Ax, values, (size_t)A.nnz, s);
            HIPCHK(hipStreamSynchronize(s));
            A.Tp.alloc(((size_t)M + 1) * 4);
            A.Ti.alloc(std::max<size_t>((size_t)A.nnz, 1) * 4);
            A.Tx.alloc(std::max<size_t>((size_t)A.nnz, 1) * 8);
            if (A.nnz > 0)
                OPCHK(rcppml_hip_transpose_csc(c, RCPPML_F64, (int)M, (int)N, A.Ap.as<int>(), A.Ai.as<int>(), A.Ax.p, A.Tp.as<int>(),
                                               A.Ti.as<int>(), A.Tx.p));
            else
                HIPCHK(hipMemsetAsync(A.Tp.p, 0, ((size_t)M + 1) * 4, s));
            A.tr.alloc(8);
            OPCHK(rcppml_hip_sumsq(c, RCPPML_F64, A.Ax.p, A.nnz, A.tr.as<double>()));
        }

        Engine E{c, s, A, layers};
        E.solver_mode = smode; E.norm_type = ntype; E.cd_maxit = cdit; E.cd_tol = cdt;
        E.planA.resize((size_t)NL); E.planT.resize((size_t)NL);
        for (int i = 0; i < NL; ++i) {
            Layer& l = layers[(size_t)i];
            const size_t kw = (size_t)l.k * (size_t)l.rows, kh = (size_t)l.k * (size_t)l.cols;
            if (st == 1) {
                upload(l.W, W + l.offW, kw, s);
                upload(l.d, d + l.offd, (size_t)l.k, s);
                upload(l.H, H + l.offH, kh, s);
            } else {
                // initialize_factors (nmf/nmf_init.hpp:166-182): one stream, W_T then H; d = 1
                const std::vector<double> w0 = splitmix<double>((uint64_t)(seed_base + (uint32_t)i), 0, kw);
                const std::vector<double> h0 = splitmix<double>((uint64_t)(seed_base + (uint32_t)i), kw, kh);
                const std::vector<double> d0((size_t)l.k, 1.0);
                upload(l.W, w0.data(), kw, s);
                upload(l.H, h0.data(), kh, s);
                upload(l.d, d0.data(), (size_t)l.k, s);
                HIPCHK(hipStreamSynchronize(s));                  // the host vectors go away
            }
            if (l.p > 0) upload(l.Z, cond_Z + l.offZ, (size_t)l.p * (size_t)l.rows, s);
            if (l.kind == SRC_INPUT && !A.dense) {
                l.Bw.alloc(kw * 8);
                if (A.nnz >= (1 << 20)) {      // the planner's own threshold of usefulness in the fit (plugin.hip)
                    plan_or_none(rcppml_hip_rhs_plan_create(c, RCPPML_F64, A.Ap.as<int>(), A.Ai.as<int>(), A.Ax.p, N, M, l.k, 0, 0, &E.planA[(size_t)i].p),
                                 E.planA[(size_t)i].p);
                    plan_or_none(rcppml_hip_rhs_plan_create(c, RCPPML_F64, A.Tp.as<int>(), A.Ti.as<int>(), A.Tx.p, M, N, l.k, 0, 0, &E.planT[(size_t)i].p),
                                 E.planT[(size_t)i].p);
                }
            }
        }
        HIPCHK(hipStreamSynchronize(s));
        E.X.alloc(std::max<size_t>((size_t)max_x, 1) * 8);
        E.Bh.alloc((size_t)GRAPH_MAX_K * (size_t)max_cols * 8);
        E.Bw.alloc((size_t)GRAPH_MAX_K * (size_t)max_rows * 8);
        E.G.alloc((size_t)GRAPH_MAX_K * GRAPH_MAX_K * 8);
        E.Gs.alloc((size_t)GRAPH_MAX_K * GRAPH_MAX_K * 8);
        E.Gwt.alloc((size_t)GRAPH_MAX_K * GRAPH_MAX_K * 8);
        E.sums.alloc((size_t)GRAPH_MAX_K * 8);
        E.loss3.alloc(4 * 8);
        E.losses.alloc((size_t)kMaxLayers * 8);
        E.total.alloc(8);
        E.trX.alloc(8);

        // ---- warm-up (fit.hpp:281-298), in topological order: a later layer reads the warmed-up H of its branches
        if (st == 0)
            for (int i = 0; i < NL; ++i) E.warm_up(i, std::min(10, maxit), tl);

        // ---- outer ALS (fit.hpp:301-354)
        double prev = std::numeric_limits<double>::infinity();
        int total_iter = 0;
        bool converged = false;
        for (int outer = 0; outer < maxit; ++outer) {
            E.counting = outer == 0;
            for (int i = 0; i < NL; ++i) E.iterate(i, E.effective_input(i), false);
            ++total_iter;
            for (int i = 0; i < NL; ++i) E.layer_loss(i);
            const double cur = E.total_loss();
            E.counting = false;
            if (std::isfinite(prev) && std::fabs(prev - cur) / (std::fabs(prev) + 1e-15) < tl) {
                converged = true;
                break;
            }
            prev = cur;
        }

        // ---- nothing is written to the caller's buffers before the device work has succeeded
        std::vector<double> hW(oW), hd(od), hH(oH), hl((size_t)NL);
        for (const Layer& l : layers) {
            HIPCHK(hipMemcpyAsync(hW.data() + l.offW, l.W.p, (size_t)l.k * (size_t)l.rows * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hd.data() + l.offd, l.d.p, (size_t)l.k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(hH.data() + l.offH, l.H.p, (size_t)l.k * (size_t)l.cols * 8, hipMemcpyDeviceToHost, s));
        }
        download(hl.data(), E.losses.as<double>(), (size_t)NL, s);
        std::copy(hW.begin(), hW.end(), W);
        std::copy(hd.begin(), hd.end(), d);
        std::copy(hH.begin(), hH.end(), H);
        std::copy(hl.begin(), hl.end(), out_layer_loss);
        *out_iter = total_iter;
        *out_converged = converged ? 1 : 0;
        *out_loss = prev;
        if (out_counts) { out_counts[0] = E.ops; out_counts[1] = E.launches; }
    });
}
