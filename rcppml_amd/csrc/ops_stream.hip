// ops_stream.hip -- panel-streamed NMF (kernels: kernels_stream.hip.h): the device ops rcppml_hip_stream_rhs_w,
// rcppml_hip_stream_gram_accum, rcppml_hip_stream_gram_finish, rcppml_hip_stream_geometry and the build-defined entry
// rcppml_gpu_nmf_streaming_ex.  It is the out-of-core fit of the reference (nmf/fit_chunked.hpp, nmf/fit_streaming_spz.hpp,
// R/nmf_thin.R:442-610) as the ALS of plugin.hip regrouped: the H half-update runs panel by panel against a fixed Gram of W, and
// the W half-update's two sums over all columns (B_W = H A^T, G_H = H H^T) are accumulated over the panels.  Neither the matrix
// nor its transpose is ever resident: W, H, B_W and the Grams stay on the device, panels pass through one panel-sized buffer,
// uploaded from a host CSC or decoded from the chunks of an .spz file (rcppml_spz_decode_columns, ops_spz.hip).
//
// Every argument is checked before the device is touched, and outputs are written only after the fit has succeeded, so a refused
// call leaves every output buffer as it was.
#include "gram_launch.hip.h"
#include "kernels_stream.hip.h"
#include "stream_panels.hip.h"

#include <limits>

namespace {
using namespace rcppml_plugin;
using namespace rstream;

template <class T, int KP>
void launch_rhs_w(rcppml_hip_ctx* c, const int* ri, const T* ax, const int* tp, int64_t pc, int64_t m, int64_t ntiles, unsigned grid,
                  const T* H, int k, int accumulate, T* BW) {
    static DynSmemOnce once;
    constexpr size_t smem = lds_bytes<T, KP>();
    once.ensure(reinterpret_cast<const void*>(stream_rhs_w_kernel<T, KP>), smem, c->device);
    hipLaunchKernelGGL((stream_rhs_w_kernel<T, KP>), dim3(grid), dim3(NT), smem, c->stream, ri, ax, tp, pc, m, ntiles, H, k, accumulate,
                       BW);
    HIPCHK(hipGetLastError());
}

template <class T>
void rhs_w_impl(rcppml_hip_ctx* c, const int* cp, const int* ri, const T* ax, int64_t pc, int64_t m, const T* H, int k, int accumulate,
                int groups, T* BW) {
    if (k < 1 || k > 64) throw std::invalid_argument("stream_rhs_w: k must be in [1, 64]");
    if (pc < 0 || m < 1 || m > INT_MAX) throw std::invalid_argument("stream_rhs_w: bad shape");
    const int KP = k_pad(k), R = tile_rows(sizeof(T), k), RW = R / NW;
    const int64_t ntiles = (m + R - 1) / R, nb = ntiles * NW;
    const int64_t cells = (nb + 1) * std::max<int64_t>(pc, 1);
    if (cells > ((int64_t)1 << 29)) throw std::invalid_argument("stream_rhs_w: the panel's range table would exceed 2 GiB; use narrower panels");
    int* tp = static_cast<int*>(c->scratch(WS_GRAPH, (size_t)cells * sizeof(int)));
    if (pc > 0) {
        hipLaunchKernelGGL(stream_tile_ptr_kernel, dim3((unsigned)(((nb + 1) * pc + 255) / 256)), dim3(256), 0, c->stream, cp, ri, pc, nb,
                           RW, tp);
        HIPCHK(hipGetLastError());
    }
    const unsigned grid = (unsigned)(groups > 0 ? std::min<int64_t>(groups, ntiles) : ntiles);
    switch (KP) {
        case 8: launch_rhs_w<T, 8>(c, ri, ax, tp, pc, m, ntiles, grid, H, k, accumulate, BW); break;
        case 16: launch_rhs_w<T, 16>(c, ri, ax, tp, pc, m, ntiles, grid, H, k, accumulate, BW); break;
        case 32: launch_rhs_w<T, 32>(c, ri, ax, tp, pc, m, ntiles, grid, H, k, accumulate, BW); break;
        default: launch_rhs_w<T, 64>(c, ri, ax, tp, pc, m, ntiles, grid, H, k, accumulate, BW); break;
    }
}

template <class T>
void gram_accum_impl(rcppml_hip_ctx* c, const T* Hp, int k, int64_t pc, int accumulate, T* Gacc) {
    if (k < 1 || k > 64) throw std::invalid_argument("stream_gram_accum: k must be in [1, 64]");
    int nblk = 0, KP = gram_kp<T>(k);
    const T* partial = Gacc;                                   // an empty panel adds nothing (nblk = 0)
    if (pc > 0) partial = gram_partials<T>(c, Hp, k, pc, &nblk, &KP);
    if (pc <= 0 && accumulate) return;
    hipLaunchKernelGGL(stream_gram_add_kernel<T>, dim3((k * k + 255) / 256), dim3(256), 0, c->stream, partial, nblk, KP, k, accumulate, Gacc);
    HIPCHK(hipGetLastError());
}

template <class T>
void gram_finish_impl(rcppml_hip_ctx* c, const T* Gacc, const T* d, int k, T eps, T l2, T* G) {
    hipLaunchKernelGGL(stream_gram_finish_kernel<T>, dim3((k * k + 255) / 256), dim3(256), 0, c->stream, Gacc, d, k, eps, l2, G);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" int rcppml_hip_stream_geometry(int dtype, int k, int64_t* out) {
    if (!out || k < 1 || k > 64 || (dtype != RCPPML_F32 && dtype != RCPPML_F64)) { rcppml_err() = "stream_geometry: k in [1, 64], dtype 0 or 1"; return 1; }
    const int R = tile_rows(dtype == RCPPML_F32 ? 4 : 8, k);
    out[0] = R; out[1] = NW; out[2] = R / NW; out[3] = k_pad(k);
    return 0;
}

extern "C" int rcppml_hip_stream_rhs_w(rcppml_hip_ctx* c, int dtype, const int* col_ptr, const int* row_idx, const void* values,
                                       int64_t ncols, int64_t nrows, const void* H_p, int k, int accumulate, int groups, void* B_W) {
    try {
        HIPCHK(hipSetDevice(c->device));
        if (dtype == RCPPML_F32) rhs_w_impl<float>(c, col_ptr, row_idx, (const float*)values, ncols, nrows, (const float*)H_p, k, accumulate, groups, (float*)B_W);
        else rhs_w_impl<double>(c, col_ptr, row_idx, (const double*)values, ncols, nrows, (const double*)H_p, k, accumulate, groups, (double*)B_W);
        return 0;
    }
    RCPPML_CATCH_RET
}

extern "C" int rcppml_hip_stream_gram_accum(rcppml_hip_ctx* c, int dtype, const void* H_p, int k, int64_t ncols, int accumulate, void* G_acc) {
    try {
        HIPCHK(hipSetDevice(c->device));
        if (dtype == RCPPML_F32) gram_accum_impl<float>(c, (const float*)H_p, k, ncols, accumulate, (float*)G_acc);
        else gram_accum_impl<double>(c, (const double*)H_p, k, ncols, accumulate, (double*)G_acc);
        return 0;
    }
    RCPPML_CATCH_RET
}

extern "C" int rcppml_hip_stream_gram_finish(rcppml_hip_ctx* c, int dtype, const void* G_acc, const void* d, int k, double eps, double l2,
                                             void* G) {
    try {
        HIPCHK(hipSetDevice(c->device));
        if (k < 1 || k > 64) throw std::invalid_argument("stream_gram_finish: k must be in [1, 64]");
        if (dtype == RCPPML_F32) gram_finish_impl<float>(c, (const float*)G_acc, (const float*)d, k, (float)eps, (float)l2, (float*)G);
        else gram_finish_impl<double>(c, (const double*)G_acc, (const double*)d, k, eps, l2, (double*)G);
        return 0;
    }
    RCPPML_CATCH_RET
}

namespace {

// bytes of the range table of rcppml_hip_stream_rhs_w for a panel of pc columns
size_t range_table_bytes(size_t elem, int k, int64_t m, int64_t pc) {
    const int R = tile_rows(elem, k);
    return (size_t)(((m + R - 1) / R) * NW + 1) * (size_t)std::max<int64_t>(pc, 1) * sizeof(int);
}

struct StreamArgs {
    const PanelSource* src = nullptr;        // the matrix and its panels (stream_panels.hip.h)
    std::vector<int64_t> pb;                 // panel q holds columns pb[q] .. pb[q + 1]
    int64_t m, n, pc;                        // pc: the widest panel's columns
    int k, max_iter, norm_type, solver_mode, cd_maxit, patience, sort_model, nonneg_W, nonneg_H;
    double tol, cd_tol, L1_W, L1_H, L2_W, L2_H, ub_W, ub_H;
    double *W, *H, *d, *loss_history;
    int out_iter = 0, out_converged = 0, ops_per_iter = 0;
    double out_loss = 0, out_tol = 0;
    const int* colptr() const { return src->colptr(); }
};

// the plain fit of plugin.hip (fit<T>, MSE branch) with the columns regrouped into panels; see the file comment
template <class T>
void fit_stream(StreamArgs& P) {
    const int dt = DT<T>::id, k = P.k;
    const int64_t m = P.m, n = P.n, np = (int64_t)P.pb.size() - 1;
    const int* cp = P.colptr();

    CtxGuard g(env_device());
    rcppml_hip_ctx* c = g.c;
    hipStream_t s = g.s;
    PanelBuffer<T> panel(*P.src, c, s);
    DevBuf &bp = panel.bp, &bi = panel.bi, &bx = panel.bx;
    constexpr bool f32 = std::is_same<T, float>::value;
    DevBuf dW, dH, dd, dBw, dBh, dG, dGs, dGacc, dGwt, dsums, dtr, dtrp, dloss;
    upload_cast<T>(c, P.W, (size_t)k * m, dW, s);
    upload_cast<T>(c, P.H, (size_t)k * n, dH, s);
    std::vector<T> ones(k, T(1));
    upload<T>(dd, ones.data(), (size_t)k, s);
    HIPCHK(hipStreamSynchronize(s));
    dalloc<T>(dBw, (size_t)k * m);
    dalloc<T>(dBh, (size_t)k * P.pc);
    for (DevBuf* b : {&dG, &dGs, &dGacc, &dGwt}) dalloc<T>(*b, (size_t)k * k);
    dalloc<T>(dsums, (size_t)k);
    dalloc<double>(dtr, 1);
    zeros<double>(dtrp, (size_t)np, s);
    dalloc<double>(dloss, 4);

    const double eps = 1e-15;
    double prev_loss = f32 ? (double)std::numeric_limits<float>::max() : std::numeric_limits<double>::max();
    double last_loss = 0, train_loss = 0, final_tol = 0;
    int patience_counter = 0, iterations = 0;
    bool converged = false;
    auto solve = [&](const void* G, const void* B, void* X, int64_t ncols, double l1, int nonneg, double ub, int warm) {
        if (P.solver_mode == 0)
            OPCHK(rcppml_hip_solve_cd(c, dt, G, B, X, k, ncols, l1 > 0 ? l1 : 0.0, warm, 0, 0.0, 0.0, nonneg, P.cd_maxit, P.cd_tol, 0.0, ub,
                                      RCPPML_CD_AUTO, nullptr, nullptr));
        else
            OPCHK(rcppml_hip_solve_chol(c, dt, G, B, X, k, ncols, l1 > 0 ? l1 : 0.0, nonneg, ub));
    };
    for (int iter = 0; iter < P.max_iter; ++iter) {
        const int warm = iter > 0 ? 1 : 0;
        int ops = 0;
        OPCHK(rcppml_hip_gram(c, dt, dW.p, k, m, eps, P.L2_H, dG.p)); ++ops;
        for (int64_t q = 0; q < np; ++q) {
            const int64_t j0 = P.pb[q], pc = P.pb[q + 1] - j0, pn = cp[P.pb[q + 1]] - cp[j0];
            panel.load(q, iter == 0);
            T* Hp = dH.as<T>() + (size_t)j0 * k;
            // H side: the panel's columns against the fixed Gram of W
            OPCHK(rcppml_hip_rhs(c, dt, bp.as<int>(), bi.as<int>(), bx.p, pc, dW.p, k, dBh.p));
            solve(dG.p, dBh.p, Hp, pc, P.L1_H, P.nonneg_H, P.ub_H, warm);
            if (iter == 0 && pn > 0) OPCHK(rcppml_hip_sumsq(c, dt, bx.p, pn, dtrp.as<double>() + q));
            // W side: the two sums over all columns, panel by panel, from the UNSCALED H (scaled once below)
            OPCHK(rcppml_hip_stream_rhs_w(c, dt, bp.as<int>(), bi.as<int>(), bx.p, pc, m, Hp, k, q > 0, 0, dBw.p));
            OPCHK(rcppml_hip_stream_gram_accum(c, dt, Hp, k, pc, q > 0, dGacc.p));
            ops += 5 + (f32 ? 1 : 0);                          // the panel load counts as one
        }
        if (iter == 0) {
            hipLaunchKernelGGL(stream_sum_kernel, dim3(1), dim3(64), 0, s, dtrp.as<double>(), (int)np, dtr.as<double>());
            HIPCHK(hipGetLastError());
        }
        // extract_scaling of H; B_W and G_H are linear / bilinear in H's rows, so the same d scales them after the fact
        OPCHK(rcppml_hip_scale_order(c, dt, dH.p, k, n, P.norm_type, dsums.p, dd.p, nullptr, nullptr));
        if (P.norm_type != 2) OPCHK(rcppml_hip_apply_scaling(c, dt, dBw.p, k, m, P.norm_type, dsums.p, dd.p));
        OPCHK(rcppml_hip_stream_gram_finish(c, dt, dGacc.p, P.norm_type != 2 ? dd.p : nullptr, k, eps, 0.0, dGs.p));
        if (P.L2_W > 0) OPCHK(rcppml_hip_stream_gram_finish(c, dt, dGacc.p, P.norm_type != 2 ? dd.p : nullptr, k, eps, P.L2_W, dG.p));
        solve(P.L2_W > 0 ? dG.p : dGs.p, dBw.p, dW.p, m, P.L1_W, P.nonneg_W, P.ub_W, warm);
        OPCHK(rcppml_hip_tail_scale_gram_loss(c, dt, dW.p, k, m, P.norm_type, dsums.p, dd.p, nullptr, nullptr, eps, dtr.as<double>(), dBw.p,
                                              dGs.p, dGwt.p, dloss.as<double>()));
        P.ops_per_iter = ops + 4 + (P.norm_type != 2 ? 1 : 0) + (P.L2_W > 0 ? 1 : 0);
        double hloss[4];
        download<double>(hloss, dloss.as<double>(), 4, s);
        double loss_val = hloss[0];
        if (f32) loss_val = static_cast<double>(static_cast<float>(loss_val));
        last_loss = loss_val;
        if (P.loss_history) P.loss_history[iter] = loss_val;
        // the convergence rule of the plain fit (fit_cpu.hpp:1769-1809)
        bool loss_converged = false;
        if (iter > 0) {
            final_tol = std::fabs(prev_loss - loss_val) / (std::fabs(prev_loss) + 1e-15);
            loss_converged = final_tol < P.tol;
        }
        prev_loss = loss_val;
        iterations = iter + 1;
        if (iter > 0) {
            if (loss_converged) {
                if (++patience_counter >= P.patience) { converged = true; train_loss = prev_loss; break; }
            } else patience_counter = 0;
        }
    }
    if (!converged) train_loss = last_loss;

    std::vector<double> hW((size_t)k * m), hH((size_t)k * n), hd((size_t)k);
    download_cast<T>(c, dW, hW.size(), hW.data(), s);
    download_cast<T>(c, dH, hH.size(), hH.data(), s);
    download_cast<T>(c, dd, hd.size(), hd.data(), s);
    std::vector<int> idx(k);
    std::iota(idx.begin(), idx.end(), 0);
    if (P.sort_model) std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return hd[a] > hd[b]; });   // core/result.hpp:169-188
    for (int f = 0; f < k; ++f) P.d[f] = hd[idx[f]];
    for (int64_t r = 0; r < m; ++r)
        for (int f = 0; f < k; ++f) P.W[(size_t)r * k + f] = hW[(size_t)r * k + idx[f]];
    for (int64_t j = 0; j < n; ++j)
        for (int f = 0; f < k; ++f) P.H[(size_t)j * k + f] = hH[(size_t)j * k + idx[f]];
    P.out_iter = iterations; P.out_converged = converged ? 1 : 0; P.out_loss = train_loss; P.out_tol = final_tol;
}

}  // namespace

extern "C" void rcppml_gpu_nmf_streaming_ex(const int* col_ptr, const int* row_idx, const double* values, int* nnz, const char* spz_path,
                                            int* m, int* n, int* k, int* panel_cols, double* W, double* H, double* d, int* max_iter,
                                            double* tol, const double* L1, const double* L2, const double* upper_bound,
                                            const int* nonneg, int* norm_type, int* solver_mode, int* cd_maxit, double* cd_tol,
                                            int* patience, int* sort_model, int* precision, int* devices, double* loss_history,
                                            int* out_iter, int* out_converged, double* out_loss, double* out_tol, int64_t* out_info,
                                            int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !n || !k || !panel_cols || !max_iter || !tol || !norm_type || !solver_mode || !cd_maxit || !cd_tol || !patience ||
            !sort_model || !precision)
            throw std::invalid_argument("null scalar argument");
        if (!L1 || !L2 || !upper_bound || !nonneg) throw std::invalid_argument("null penalty argument");
        if (!W || !H || !d || !out_iter || !out_converged || !out_loss || !out_tol || !out_info) throw std::invalid_argument("null output");
        if (spz_path && col_ptr) throw std::invalid_argument("data: pass host CSC arrays or an .spz path, not both");
        if (devices && *devices > 1) throw std::invalid_argument("devices > 1: the streamed fit runs on one device");
        if (*m < 1 || *n < 1) throw std::invalid_argument("m and n must be >= 1");
        if (*k < 1) throw std::invalid_argument("k must be >= 1");
        if (*k > 64) throw std::invalid_argument("k > 64: the streamed fit's kernels serve ranks up to 64");
        if (*panel_cols < 0) throw std::invalid_argument("panel_cols must be >= 0 (0 = automatic)");
        if (*max_iter < 1) throw std::invalid_argument("max_iter must be >= 1");
        if (*precision != RCPPML_F32 && *precision != RCPPML_F64) throw std::invalid_argument("precision must be 0 (fp32) or 1 (fp64)");
        if (*solver_mode != 0 && *solver_mode != 1) throw std::invalid_argument("solver_mode must be 0 (CD) or 1 (Cholesky + clip)");
        if (*norm_type < 0 || *norm_type > 2) throw std::invalid_argument("norm_type must be 0 (L1), 1 (L2) or 2 (none)");
        StreamArgs P{};
        P.m = *m; P.n = *n; P.k = *k;
        PanelSource src;
        if (spz_path) src.open_spz(spz_path, P.m, P.n);
        else src.open_csc(col_ptr, row_idx, values, nnz, P.m, P.n);
        all_finite(W, (size_t)*k * *m, "W");
        all_finite(H, (size_t)*k * *n, "H");
        const size_t el = *precision == RCPPML_F32 ? 4 : 8;
        // panel_cols = 0: panels of about 64 MiB of CSC at the matrix's mean column size, in whole multiples of 256 columns, and no
        // wider than the range table of stream_rhs_w allows (2^29 cells)
        const int64_t cap = std::max<int64_t>(1, (((int64_t)1 << 29) * 4) / (int64_t)range_table_bytes(el, P.k, P.m, 1));
        src.plan(*panel_cols, cap);
        P.src = &src; P.pb = src.pb; P.pc = src.pc;
        if (P.pc > cap) throw std::invalid_argument("panel_cols: the range table of the W-side kernel would exceed 2 GiB at " + std::to_string(P.pc) +
                                                    " columns per panel; use at most " + std::to_string(cap));
        P.max_iter = *max_iter; P.tol = *tol; P.norm_type = *norm_type; P.solver_mode = *solver_mode; P.cd_maxit = *cd_maxit;
        P.cd_tol = *cd_tol; P.patience = *patience; P.sort_model = *sort_model;
        P.L1_W = L1[0]; P.L1_H = L1[1]; P.L2_W = L2[0]; P.L2_H = L2[1]; P.ub_W = upper_bound[0]; P.ub_H = upper_bound[1];
        P.nonneg_W = nonneg[0]; P.nonneg_H = nonneg[1];
        P.W = W; P.H = H; P.d = d; P.loss_history = loss_history;
        const size_t panel_bytes = src.buffer_bytes(el), table_bytes = range_table_bytes(el, P.k, P.m, P.pc);
        // factors, right-hand sides and the cast staging of the factors; the panel buffer; the range table; .spz: the decoder's scratch
        device_ready(el * (size_t)P.k * (size_t)(2 * P.m + P.n + P.pc) + 8 * (size_t)P.k * (size_t)std::max(P.m, P.n) + panel_bytes + table_bytes +
                         src.decode_bytes() + ((size_t)64 << 20),
                     "the streamed fit");
        if (*precision == RCPPML_F32) fit_stream<float>(P);
        else fit_stream<double>(P);
        *out_iter = P.out_iter; *out_converged = P.out_converged; *out_loss = P.out_loss; *out_tol = P.out_tol;
        out_info[0] = (int64_t)P.pb.size() - 1; out_info[1] = P.pc; out_info[2] = (int64_t)panel_bytes; out_info[3] = P.ops_per_iter;
        out_info[4] = (int64_t)table_bytes;
    });
}
