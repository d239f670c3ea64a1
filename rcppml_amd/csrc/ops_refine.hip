// ops_refine.hip -- label-guided refinement: the reference's compute_target() (R/compute_target.R:65-121) and refine()
// (R/refine.R:109-187, without a batch) on the device, fp64.  Build-defined entries: R has no hook for them.
//
// What runs where.  The label-dependent O(k n) passes are kernels (kernels_refine.hip.h): the per-class centroid sums over a
// host-built class permutation, ||H||_F^2, and the fused correction H_corr = H + lambda s T with the clip.  The k x C stage between
// them (centroids, the OAS-shrunk covariance, its eigendecomposition by cyclic Jacobi, the ZCA matrix, the shifts and
// ||T||_F^2 = sum_c count_c ||shift_c||^2) is host C++ on k x C numbers: k C + 1 doubles come down and k C go up per evaluation.
// The W-refit cycle of refine() runs on the device-level ops of the fit (Gram, right-hand sides on A and on its device-side
// transpose, Cholesky solve with an optional clip, row norms); no k x n or k x m array returns to the host between cycles.
//
// The solves are R's solve(G + 1e-8 I, B) followed by a clip: the ridge goes into the Gram (rcppml_hip_gram's eps) and
// rcppml_hip_solve_chol's nonneg flag is the clip.  They are not NNLS.
//
// Edge cases where R is undefined: with no labelled column at all (sum(counts) = 0) the whitening is skipped (R divides by zero);
// the target is zero either way.
#include "entry_common.hip.h"
#include "kernels_refine.hip.h"

#include <cmath>
#include <limits>
#include <string>
#include <vector>

namespace {
using namespace rcppml_plugin;
using namespace rref;

unsigned grid_for(int64_t total) {
    const int64_t b = (total + NT - 1) / NT;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(b, 8192));
}

// ------------------------------------------------------------------------------------------------------------------ labels
// counts, the class permutation (a stable counting sort of the labelled columns) and its chunks
struct Labels {
    int64_t n = 0;
    int C = 0;
    std::vector<int> counts, perm, chunk_start, chunk_len, class_chunk_ptr;
    int64_t labelled = 0;
    Labels(const int* labels, int64_t n_, int C_) : n(n_), C(C_) {
        counts.assign((size_t)C, 0);
        for (int64_t j = 0; j < n; ++j) {
            if (labels[j] >= C) throw std::invalid_argument("a label is >= n_classes (labels are 0 .. n_classes - 1, negative = NA)");
            if (labels[j] >= 0) { ++counts[(size_t)labels[j]]; ++labelled; }
        }
        std::vector<int64_t> at((size_t)C + 1, 0);
        for (int c = 0; c < C; ++c) at[(size_t)c + 1] = at[(size_t)c] + counts[(size_t)c];
        class_chunk_ptr.assign((size_t)C + 1, 0);
        for (int c = 0; c < C; ++c) {
            for (int64_t o = 0; o < counts[(size_t)c]; o += CHUNK) {
                chunk_start.push_back((int)(at[(size_t)c] + o));
                chunk_len.push_back((int)std::min<int64_t>(CHUNK, counts[(size_t)c] - o));
            }
            class_chunk_ptr[(size_t)c + 1] = (int)chunk_start.size();
        }
        perm.resize((size_t)labelled);
        for (int64_t j = 0; j < n; ++j)
            if (labels[j] >= 0) perm[(size_t)at[(size_t)labels[j]]++] = (int)j;
    }
};

// ------------------------------------------------------------------------------------------------------------ k x C stage
// Symmetric eigendecomposition by cyclic Jacobi: A (k x k, column-major) is overwritten, its diagonal holds the eigenvalues and V
// (k x k, column-major) the eigenvectors as columns.
void jacobi_eigen(std::vector<double>& A, std::vector<double>& V, int k) {
    V.assign((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i) V[(size_t)i * k + i] = 1.0;
    auto a = [&](int r, int c) -> double& { return A[(size_t)c * k + r]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0, all = 0;
        for (int c = 0; c < k; ++c)
            for (int r = 0; r < k; ++r) {
                all += a(r, c) * a(r, c);
                if (r != c) off += a(r, c) * a(r, c);
            }
        if (off == 0.0 || off <= 1e-40 * all) break;
        for (int p = 0; p < k - 1; ++p)
            for (int q = p + 1; q < k; ++q) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double theta = (a(q, q) - a(p, p)) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int r = 0; r < k; ++r) {                 // columns p, q
                    const double x = a(r, p), y = a(r, q);
                    a(r, p) = cs * x - sn * y;
                    a(r, q) = sn * x + cs * y;
                }
                for (int c = 0; c < k; ++c) {                 // rows p, q
                    const double x = a(p, c), y = a(q, c);
                    a(p, c) = cs * x - sn * y;
                    a(q, c) = sn * x + cs * y;
                }
                a(p, q) = 0.0; a(q, p) = 0.0;
                for (int r = 0; r < k; ++r) {
                    const double x = V[(size_t)p * k + r], y = V[(size_t)q * k + r];
                    V[(size_t)p * k + r] = cs * x - sn * y;
                    V[(size_t)q * k + r] = sn * x + cs * y;
                }
            }
    }
}

// R/compute_target.R:76-115 from the class sums: shift (k x C) and ||T||_F^2
void shifts_from_sums(const std::vector<double>& sums, const std::vector<int>& counts, int k, int C, bool whiten,
                      std::vector<double>& shift, double& tnorm2) {
    std::vector<double> cen((size_t)k * C, 0.0), gm((size_t)k, 0.0);
    int nonempty = 0;
    double n_eff = 0;
    for (int c = 0; c < C; ++c) {
        if (counts[(size_t)c] > 0) {
            ++nonempty;
            for (int f = 0; f < k; ++f) cen[(size_t)c * k + f] = sums[(size_t)c * k + f] / (double)counts[(size_t)c];
        }
        n_eff += (double)counts[(size_t)c];
    }
    // rowMeans over the non-empty classes (0 / 0 = NaN without one, as in R; no column reads the shifts then)
    for (int f = 0; f < k; ++f) {
        double s = 0;
        for (int c = 0; c < C; ++c)
            if (counts[(size_t)c] > 0) s += cen[(size_t)c * k + f];
        gm[(size_t)f] = s / (double)nonempty;
    }
    if (whiten && C > 1 && n_eff > 0) {
        std::vector<double> X((size_t)k * C), S((size_t)k * k, 0.0);
        for (int c = 0; c < C; ++c) {
            const double w = std::sqrt((double)std::max(counts[(size_t)c], 1));
            for (int f = 0; f < k; ++f) X[(size_t)c * k + f] = (cen[(size_t)c * k + f] - gm[(size_t)f]) * w;
        }
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < k; ++i) {
                double s = 0;
                for (int c = 0; c < C; ++c) s += X[(size_t)c * k + i] * X[(size_t)c * k + j];
                S[(size_t)j * k + i] = s / n_eff;
            }
        double trS = 0, trS2 = 0;
        for (int i = 0; i < k; ++i) trS += S[(size_t)i * k + i];
        for (double v : S) trS2 += v * v;
        const double kk = (double)k;
        const double rho_num = (1.0 - 2.0 / kk) * trS2 + trS * trS;
        const double rho_den = (n_eff + 1.0 - 2.0 / kk) * (trS2 - trS * trS / kk);
        const double rho = std::fabs(rho_den) < 1e-12 ? 1.0 : std::min(1.0, std::max(0.0, rho_num / rho_den));
        for (double& v : S) v *= (1.0 - rho);
        for (int i = 0; i < k; ++i) S[(size_t)i * k + i] += rho * (trS / kk);
        std::vector<double> V;
        jacobi_eigen(S, V, k);
        std::vector<double> Wz((size_t)k * k, 0.0);
        for (int e = 0; e < k; ++e) {
            const double val = std::max(S[(size_t)e * k + e], 1e-10);
            const double is = 1.0 / std::sqrt(val);
            for (int j = 0; j < k; ++j)
                for (int i = 0; i < k; ++i) Wz[(size_t)j * k + i] += V[(size_t)e * k + i] * is * V[(size_t)e * k + j];
        }
        std::vector<double> cen2((size_t)k * C, 0.0), gm2((size_t)k, 0.0);
        for (int c = 0; c < C; ++c)
            for (int i = 0; i < k; ++i) {
                double s = 0;
                for (int j = 0; j < k; ++j) s += Wz[(size_t)j * k + i] * cen[(size_t)c * k + j];
                cen2[(size_t)c * k + i] = s;
            }
        for (int i = 0; i < k; ++i) {
            double s = 0;
            for (int j = 0; j < k; ++j) s += Wz[(size_t)j * k + i] * gm[(size_t)j];
            gm2[(size_t)i] = s;
        }
        cen.swap(cen2);
        gm.swap(gm2);
    }
    shift.assign((size_t)k * C, 0.0);
    tnorm2 = 0;
    for (int c = 0; c < C; ++c) {
        double s = 0;
        for (int f = 0; f < k; ++f) {
            const double v = cen[(size_t)c * k + f] - gm[(size_t)f];
            shift[(size_t)c * k + f] = v;
            s += v * v;
        }
        if (counts[(size_t)c] > 0) tnorm2 += (double)counts[(size_t)c] * s;
    }
}

// ------------------------------------------------------------------------------------------------- the target stage on the device
struct TargetStage {
    const Labels& L;
    int k;
    int64_t n;
    bool whiten;
    hipStream_t s;
    DevBuf dLab, dPerm, dStart, dLen, dPtr, dPartial, dSums, dSqPart, dTable;
    int64_t sq_chunks;
    std::vector<double> shift;          // the last evaluation's k x C shifts (unscaled)
    static size_t bytes(const Labels& L, int k, int64_t n) {
        const size_t kc = (size_t)k * (size_t)std::max(L.C, 1);
        return 4 * (size_t)(n + L.labelled + 2 * (int64_t)L.chunk_start.size() + L.C + 1) + 8 * (L.chunk_start.size() * (size_t)k) +
               16 * kc + 8 * (size_t)(((int64_t)k * n + SQ_CHUNK - 1) / SQ_CHUNK) + 4096;
    }
    TargetStage(const Labels& L_, const int* labels, int k_, int64_t n_, bool whiten_, hipStream_t s_)
        : L(L_), k(k_), n(n_), whiten(whiten_), s(s_) {
        upload(dLab, labels, (size_t)n, s);
        upload(dPerm, L.perm.data(), L.perm.size(), s);
        upload(dStart, L.chunk_start.data(), L.chunk_start.size(), s);
        upload(dLen, L.chunk_len.data(), L.chunk_len.size(), s);
        upload(dPtr, L.class_chunk_ptr.data(), L.class_chunk_ptr.size(), s);
        HIPCHK(hipStreamSynchronize(s));          // these copies, and the caller's uploads queued before them, have landed
        dPartial.alloc(std::max<size_t>(L.chunk_start.size() * (size_t)k, 1) * 8);
        dSums.alloc(((size_t)k * L.C + 1) * 8);
        dTable.alloc(std::max<size_t>((size_t)k * L.C, 1) * 8);
        sq_chunks = ((int64_t)k * n + SQ_CHUNK - 1) / SQ_CHUNK;
        dSqPart.alloc((size_t)sq_chunks * 8);
    }
    void add_table(const double* dH, const std::vector<double>& table, int nonneg, double* dOut) {
        const size_t kc = (size_t)k * L.C;
        if (kc) {
            HIPCHK(hipMemcpyAsync(dTable.p, table.data(), kc * 8, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        const unsigned g = grid_for((int64_t)k * n);
        if (kc && kc * 8 <= TABLE_LDS_MAX)
            hipLaunchKernelGGL(add_table_kernel<true>, dim3(g), dim3(NT), kc * 8, s, dH, dLab.as<int>(), dTable.as<double>(), k, L.C, n,
                               nonneg, dOut);
        else
            hipLaunchKernelGGL(add_table_kernel<false>, dim3(g), dim3(NT), 0, s, dH, dLab.as<int>(), dTable.as<double>(), k, L.C, n,
                               nonneg, dOut);
        HIPCHK(hipGetLastError());
    }
    // the shifts of dH (kept in `shift`); with dCorr: dCorr = clip(dH + lambda s T); with dTarget: dTarget = T
    void run(const double* dH, double lambda, int nonneg, double* dCorr, double* dTarget) {
        const size_t kc = (size_t)k * L.C;
        const size_t nchunks = L.chunk_start.size();
        if (nchunks)
            hipLaunchKernelGGL(centroid_partial_kernel, dim3((unsigned)nchunks), dim3(NT), 0, s, dH, k, dPerm.as<int>(), dStart.as<int>(),
                               dLen.as<int>(), dPartial.as<double>());
        if (kc)
            hipLaunchKernelGGL(centroid_final_kernel, dim3((unsigned)((kc + NT - 1) / NT)), dim3(NT), 0, s, dPartial.as<double>(), k, L.C,
                               dPtr.as<int>(), dSums.as<double>());
        HIPCHK(hipGetLastError());
        if (dCorr) {
            hipLaunchKernelGGL(sumsq_chunk_kernel, dim3((unsigned)sq_chunks), dim3(NT), 0, s, dH, (int64_t)k * n, dSqPart.as<double>());
            hipLaunchKernelGGL(sum_chunks_kernel, dim3(1), dim3(NT), 0, s, dSqPart.as<double>(), sq_chunks, dSums.as<double>() + kc);
            HIPCHK(hipGetLastError());
        }
        std::vector<double> sums(kc + 1, 0.0);
        download(sums.data(), dSums.as<double>(), dCorr ? kc + 1 : kc, s);
        const double hsq = sums[kc];
        sums.resize(kc);
        double tn2 = 0;
        shifts_from_sums(sums, L.counts, k, L.C, whiten, shift, tn2);
        if (dTarget) add_table(nullptr, shift, 0, dTarget);
        if (dCorr) {
            // R/refine.R:114-119: target * (fro_H / fro_T) when fro_T > 1e-10, then H + lambda * target
            const double fro_H = std::sqrt(hsq), fro_T = std::sqrt(tn2);
            std::vector<double> table(kc);
            for (size_t e = 0; e < kc; ++e) {
                const double t = fro_T > 1e-10 ? shift[e] * (fro_H / fro_T) : shift[e];
                table[e] = lambda * t;
            }
            add_table(dH, table, nonneg, dCorr);
        }
    }
};

// ------------------------------------------------------------------------------------------------------------ argument checks
struct Dims { int k; int64_t n; int C; };
Dims read_dims(const int* k, const int* n, const int* n_classes) {
    if (!k || !n || !n_classes) throw std::invalid_argument("null scalar argument");
    if (*k < 1) throw std::invalid_argument("k must be >= 1");
    if (*n < 1) throw std::invalid_argument("n must be >= 1");
    if (*n_classes < 0) throw std::invalid_argument("n_classes must be >= 0");
    if ((int64_t)*k * (int64_t)std::max(*n_classes, 1) >= ((int64_t)1 << 31)) throw std::invalid_argument("k * n_classes is too large");
    return Dims{*k, (int64_t)*n, *n_classes};
}
void check_lambda(const double* lambda) {
    if (!lambda) throw std::invalid_argument("null lambda");
    if (!(*lambda >= 0.0 && *lambda <= 1.0)) throw std::invalid_argument("lambda must be in [0, 1]");
}

// The matrix of the refit: a host CSC or a column-major dense array, exactly one of the two.
struct MatIn {
    const int* p = nullptr; const int* i = nullptr; const double* x = nullptr;
    int64_t nnz = 0;
    const double* dense = nullptr;
    int64_t m = 0, n = 0;
};
MatIn read_matrix(const int* col_ptr, const int* row_idx, const double* values, const int* nnz, const double* dense, int64_t m,
                  int64_t n) {
    if (col_ptr && dense) throw std::invalid_argument("give the matrix either as a CSC or as a dense array, not both");
    if (!col_ptr && !dense) throw std::invalid_argument("give the matrix as a CSC or as a dense array");
    MatIn in;
    in.m = m; in.n = n;
    if (col_ptr) {
        if (!nnz || *nnz < 0) throw std::invalid_argument("nnz must be >= 0");
        if (*nnz > 0 && (!row_idx || !values)) throw std::invalid_argument("null CSC array");
        in.p = col_ptr; in.i = row_idx; in.x = values; in.nnz = *nnz;
        check_csc_strict(col_ptr, row_idx, m, n, in.nnz);
        all_finite(values, (size_t)in.nnz, "the matrix");
    } else {
        in.dense = dense;
        all_finite(dense, (size_t)(m * n), "the matrix");
    }
    return in;
}
size_t matrix_bytes(const MatIn& in) {
    return in.dense ? 8 * (size_t)(in.m * in.n) : 2 * ((size_t)(in.m + in.n + 2) * 4 + (size_t)in.nnz * 12);
}

struct Plan {
    rcppml_rhs_plan* p = nullptr;
    ~Plan() { if (p) rcppml_hip_rhs_plan_destroy(p); }
};

// A on the device with what both right-hand sides need: the CSC and its device-side transpose (plans on both for large inputs),
// or the dense array.
struct DevMatrix {
    rcppml_hip_ctx* c;
    const MatIn& in;
    int k;
    DevBuf Ap, Ai, Ax, Tp, Ti, Tx, X;
    Plan planA, planT;
    DevMatrix(rcppml_hip_ctx* c_, const MatIn& in_, int k_, hipStream_t s) : c(c_), in(in_), k(k_) {
        if (in.dense) {
            upload(X, in.dense, (size_t)(in.m * in.n), s);
            HIPCHK(hipStreamSynchronize(s));
            return;
        }
        upload(Ap, in.p, (size_t)in.n + 1, s);
        upload(Ai, in.i, (size_t)in.nnz, s);
        upload(Ax, in.x, (size_t)in.nnz, s);
        HIPCHK(hipStreamSynchronize(s));
        Tp.alloc(((size_t)in.m + 1) * 4);
        Ti.alloc(std::max<size_t>((size_t)in.nnz, 1) * 4);
        Tx.alloc(std::max<size_t>((size_t)in.nnz, 1) * 8);
        if (in.nnz > 0) {
            OPCHK(rcppml_hip_transpose_csc(c, RCPPML_F64, (int)in.m, (int)in.n, Ap.as<int>(), Ai.as<int>(), Ax.p, Tp.as<int>(),
                                           Ti.as<int>(), Tx.p));
        } else {
            HIPCHK(hipMemsetAsync(Tp.p, 0, ((size_t)in.m + 1) * 4, s));
        }
        if (in.nnz >= (1 << 20)) {        // the planner's own threshold of usefulness in the fit (plugin.hip)
            plan_or_none(rcppml_hip_rhs_plan_create(c, RCPPML_F64, Ap.as<int>(), Ai.as<int>(), Ax.p, in.n, in.m, k, 0, 0, &planA.p), planA.p);
            plan_or_none(rcppml_hip_rhs_plan_create(c, RCPPML_F64, Tp.as<int>(), Ti.as<int>(), Tx.p, in.m, in.n, k, 0, 0, &planT.p), planT.p);
        }
    }
    // B (k x n) = F (k x m) A
    void rhs_cols(const void* F, void* B) {
        if (in.dense) OPCHK(rcppml_hip_rhs_dense(c, RCPPML_F64, X.p, in.m, in.n, 0, F, k, B));
        else if (planA.p) OPCHK(rcppml_hip_rhs_planned(c, planA.p, F, B));
        else OPCHK(rcppml_hip_rhs(c, RCPPML_F64, Ap.as<int>(), Ai.as<int>(), Ax.p, in.n, F, k, B));
    }
    // B (k x m) = F (k x n) A^T
    void rhs_rows(const void* F, void* B) {
        if (in.dense) OPCHK(rcppml_hip_rhs_dense(c, RCPPML_F64, X.p, in.m, in.n, 1, F, k, B));
        else if (planT.p) OPCHK(rcppml_hip_rhs_planned(c, planT.p, F, B));
        else OPCHK(rcppml_hip_rhs(c, RCPPML_F64, Tp.as<int>(), Ti.as<int>(), Tx.p, in.m, F, k, B));
    }
};

constexpr double kRidge = 1e-8;        // R/refine.R:144, :165

// W = clip(solve(G + 1e-8 I, B)) with dH = diag(d) H_corr, G = dH dH^T, B = A dH^T (R/refine.R:137-145)
void refit_W(rcppml_hip_ctx* c, DevMatrix& A, int k, int64_t m, int64_t n, const void* dHcorr, const void* dd, int nonneg,
             DevBuf& dHd, DevBuf& dG, DevBuf& dBw, void* dW) {
    OPCHK(rcppml_hip_mul_rows(c, RCPPML_F64, dHcorr, k, n, dd, dHd.p));
    OPCHK(rcppml_hip_gram(c, RCPPML_F64, dHd.p, k, n, kRidge, 0.0, dG.p));
    A.rhs_rows(dHd.p, dBw.p);
    OPCHK(rcppml_hip_solve_chol(c, RCPPML_F64, dG.p, dBw.p, dW, k, m, 0.0, nonneg, 0.0));
}

void check_refit_rank(int k) {
    if (k > 64) throw std::invalid_argument("the refit needs k <= 64 (the fp64 Cholesky solve)");
}

}  // namespace

extern "C" void rcppml_gpu_compute_target_double(const double* H, const int* labels, int* k, int* n, int* n_classes, int* whiten,
                                                 double* out_target, double* out_shift, int* out_counts, int* out_status) {
    entry_guard(out_status, [&] {
        const Dims D = read_dims(k, n, n_classes);
        if (!whiten) throw std::invalid_argument("null scalar argument");
        if (!H) throw std::invalid_argument("null H");
        if (!labels) throw std::invalid_argument("null labels");
        if (!out_target) throw std::invalid_argument("null out_target");
        all_finite(H, (size_t)D.k * (size_t)D.n, "H");
        const Labels L(labels, D.n, D.C);
        device_ready(16 * (size_t)D.k * (size_t)D.n + TargetStage::bytes(L, D.k, D.n));
        CtxGuard g(env_device());
        DevBuf dH, dT;
        upload(dH, H, (size_t)D.k * (size_t)D.n, g.s);
        dT.alloc((size_t)D.k * (size_t)D.n * 8);
        TargetStage ts(L, labels, D.k, D.n, *whiten != 0, g.s);
        ts.run(dH.as<double>(), 0.0, 0, nullptr, dT.as<double>());
        // nothing is written to the caller's buffers before the device work has succeeded
        HIPCHK(hipStreamSynchronize(g.s));
        HIPCHK(hipMemcpy(out_target, dT.p, (size_t)D.k * (size_t)D.n * 8, hipMemcpyDeviceToHost));
        if (out_shift) std::copy(ts.shift.begin(), ts.shift.end(), out_shift);
        if (out_counts) std::copy(L.counts.begin(), L.counts.end(), out_counts);
    });
}

extern "C" void rcppml_gpu_refine_correct_double(const double* H, const int* labels, int* k, int* n, int* n_classes, int* whiten,
                                                 double* lambda, int* nonneg, double* out_H_corr, double* out_target,
                                                 int* out_status) {
    entry_guard(out_status, [&] {
        const Dims D = read_dims(k, n, n_classes);
        if (!whiten || !nonneg) throw std::invalid_argument("null scalar argument");
        check_lambda(lambda);
        if (!H) throw std::invalid_argument("null H");
        if (!labels) throw std::invalid_argument("null labels");
        if (!out_H_corr) throw std::invalid_argument("null out_H_corr");
        all_finite(H, (size_t)D.k * (size_t)D.n, "H");
        const Labels L(labels, D.n, D.C);
        const size_t kn = (size_t)D.k * (size_t)D.n;
        device_ready(24 * kn + TargetStage::bytes(L, D.k, D.n));
        CtxGuard g(env_device());
        DevBuf dH, dC, dT;
        upload(dH, H, kn, g.s);
        dC.alloc(kn * 8);
        if (out_target) dT.alloc(kn * 8);
        TargetStage ts(L, labels, D.k, D.n, *whiten != 0, g.s);
        ts.run(dH.as<double>(), *lambda, *nonneg != 0, dC.as<double>(), out_target ? dT.as<double>() : nullptr);
        HIPCHK(hipStreamSynchronize(g.s));
        HIPCHK(hipMemcpy(out_H_corr, dC.p, kn * 8, hipMemcpyDeviceToHost));
        if (out_target) HIPCHK(hipMemcpy(out_target, dT.p, kn * 8, hipMemcpyDeviceToHost));
    });
}

extern "C" void rcppml_gpu_refine_wfit_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
                                              const double* dense, int* m, int* n, int* k, const double* d, const double* H_corr,
                                              int* nonneg, double* out_W, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !n || !k || !nonneg) throw std::invalid_argument("null scalar argument");
        if (*m < 1 || *n < 1 || *k < 1) throw std::invalid_argument("m, n and k must be >= 1");
        check_refit_rank(*k);
        if (!d) throw std::invalid_argument("null d");
        if (!H_corr) throw std::invalid_argument("null H_corr");
        if (!out_W) throw std::invalid_argument("null out_W");
        const int K = *k;
        const int64_t M = *m, N = *n;
        const MatIn in = read_matrix(col_ptr, row_idx, values, nnz, dense, M, N);
        all_finite(d, (size_t)K, "d");
        all_finite(H_corr, (size_t)K * (size_t)N, "H_corr");
        device_ready(matrix_bytes(in) + 8 * (size_t)K * (size_t)(2 * N + 2 * M + K + 1) + 65536);
        CtxGuard g(env_device());
        DevMatrix A(g.c, in, K, g.s);
        DevBuf dHc, dd, dHd((size_t)K * N * 8), dG((size_t)K * K * 8), dBw((size_t)K * M * 8), dW((size_t)K * M * 8);
        upload(dHc, H_corr, (size_t)K * (size_t)N, g.s);
        upload(dd, d, (size_t)K, g.s);
        HIPCHK(hipStreamSynchronize(g.s));
        refit_W(g.c, A, K, M, N, dHc.p, dd.p, *nonneg != 0, dHd, dG, dBw, dW.p);
        HIPCHK(hipStreamSynchronize(g.s));
        HIPCHK(hipMemcpy(out_W, dW.p, (size_t)K * (size_t)M * 8, hipMemcpyDeviceToHost));
    });
}

extern "C" void rcppml_gpu_refine_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz, const double* dense,
                                         int* m, int* n, int* k, const double* W_T, const double* d, const double* H,
                                         const int* labels, int* n_classes, double* lambda, int* cycles, int* nonneg, int* whiten,
                                         double* out_W, double* out_d, double* out_H, double* out_H_corr, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m) throw std::invalid_argument("null scalar argument");
        if (*m < 1) throw std::invalid_argument("m must be >= 1");
        const Dims D = read_dims(k, n, n_classes);
        if (!cycles || !nonneg || !whiten) throw std::invalid_argument("null scalar argument");
        check_lambda(lambda);
        if (*cycles < 0) throw std::invalid_argument("cycles must be >= 0");
        if (!W_T || !d || !H) throw std::invalid_argument("null model array");
        if (!labels) throw std::invalid_argument("null labels");
        if (!out_W || !out_d || !out_H || !out_H_corr) throw std::invalid_argument("null output");
        if (*cycles > 0) check_refit_rank(D.k);
        const int K = D.k;
        const int64_t M = *m, N = D.n;
        // without cycles the matrix is not needed: it may be absent, and is checked when it is there
        MatIn in;
        if (*cycles > 0 || col_ptr || dense) in = read_matrix(col_ptr, row_idx, values, nnz, dense, M, N);
        all_finite(W_T, (size_t)K * (size_t)M, "W");
        all_finite(d, (size_t)K, "d");
        all_finite(H, (size_t)K * (size_t)N, "H");
        const Labels L(labels, N, D.C);
        const size_t kn = (size_t)K * (size_t)N, km = (size_t)K * (size_t)M;
        device_ready((*cycles > 0 ? matrix_bytes(in) : 0) + 8 * (4 * kn + 2 * km + (size_t)K * (K + 2)) +
                     TargetStage::bytes(L, K, N) + 65536);
        CtxGuard g(env_device());
        rcppml_hip_ctx* c = g.c;
        DevBuf dW, dd, dH, dHc(kn * 8);
        upload(dW, W_T, km, g.s);
        upload(dd, d, (size_t)K, g.s);
        upload(dH, H, kn, g.s);
        TargetStage ts(L, labels, K, N, *whiten != 0, g.s);
        ts.run(dH.as<double>(), *lambda, *nonneg != 0, dHc.as<double>(), nullptr);
        if (*cycles > 0) {
            DevMatrix A(c, in, K, g.s);
            DevBuf dHd(kn * 8), dG((size_t)K * K * 8), dBw(km * 8), dBh(kn * 8), dss((size_t)K * 8);
            for (int cyc = 0; cyc < *cycles; ++cyc) {
                refit_W(c, A, K, M, N, dHc.p, dd.p, *nonneg != 0, dHd, dG, dBw, dW.p);
                // H = clip(solve(W^T W + 1e-8 I, W^T A)) (R/refine.R:159-166)
                OPCHK(rcppml_hip_gram(c, RCPPML_F64, dW.p, K, M, kRidge, 0.0, dG.p));
                A.rhs_cols(dW.p, dBh.p);
                OPCHK(rcppml_hip_solve_chol(c, RCPPML_F64, dG.p, dBh.p, dH.p, K, N, 0.0, *nonneg != 0, 0.0));
                // d = the row norms of H floored at 1e-10; H / d; W * d (:169-172)
                OPCHK(rcppml_hip_row_norms(c, RCPPML_F64, dH.p, K, N, 1, dss.p));
                hipLaunchKernelGGL(norm_floor_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, g.s, dss.as<double>(), K, 1e-10,
                                   dd.as<double>());
                hipLaunchKernelGGL(scale_rows_kernel<true>, dim3(grid_for((int64_t)kn)), dim3(NT), 0, g.s, dH.as<double>(), K, (int64_t)kn,
                                   dd.as<double>());
                hipLaunchKernelGGL(scale_rows_kernel<false>, dim3(grid_for((int64_t)km)), dim3(NT), 0, g.s, dW.as<double>(), K, (int64_t)km,
                                   dd.as<double>());
                HIPCHK(hipGetLastError());
                ts.run(dH.as<double>(), *lambda, *nonneg != 0, dHc.as<double>(), nullptr);
            }
        }
        // nothing is written to the caller's buffers before the device work has succeeded
        std::vector<double> hW(km), hd((size_t)K), hH(kn), hC(kn);
        download(hW.data(), dW.as<double>(), km, g.s);
        download(hd.data(), dd.as<double>(), (size_t)K, g.s);
        download(hH.data(), dH.as<double>(), kn, g.s);
        download(hC.data(), dHc.as<double>(), kn, g.s);
        std::copy(hW.begin(), hW.end(), out_W);
        std::copy(hd.begin(), hd.end(), out_d);
        std::copy(hH.begin(), hH.end(), out_H);
        std::copy(hC.begin(), hC.end(), out_H_corr);
    });
}
