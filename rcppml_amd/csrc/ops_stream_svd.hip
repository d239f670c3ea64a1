// ops_stream_svd.hip -- panel-streamed randomized SVD / PCA (kernels: kernels_stream_svd.hip.h): the device ops
// rcppml_hip_stream_block_prod and rcppml_hip_stream_block_geometry and the build-defined entry rcppml_gpu_svd_streaming_ex.  It is
// the reference's out-of-core SVD (svd/streaming.hpp:683-773, svd/streaming_matvec.hpp) for the randomized block method: the steps
// of Engine::randomized (ops_svd.hip; tests/svd_rand_ref.py is the spec) with the two products taken panel by panel.  Neither the
// matrix nor its transpose is resident: the two l-wide blocks, their records and the row means stay on the device, panels pass
// through one buffer (stream_panels.hip.h).  A pass over the matrix is one product: 2 q + 2 of them, one more for the row means.
//
// Every argument is checked before the device is touched, and outputs are written only after the fit has succeeded.
#include "kernels_stream_svd.hip.h"
#include "stream_panels.hip.h"

#include <limits>

namespace {
using namespace rcppml_plugin;
using namespace rstream_svd;

// the instantiation of a block kernel f<T, W> for w <= 128 columns (as ops_svd.hip)
#define RSV_BY_WIDTH(f, w) ((w) <= 16 ? f<T, 1> : (w) <= 32 ? f<T, 2> : (w) <= 64 ? f<T, 4> : f<T, 8>)

// cells of the range table per panel column: one per slice boundary
int64_t table_rows(int64_t m, int l) {
    const int64_t R = sb_tile_rows(l);
    return (m + R - 1) / R * NW + 1;
}

template <class T>
void block_prod_impl(rcppml_hip_ctx* c, const int* cp, const int* ri, const T* ax, int64_t m, int64_t pc, int l, const T* X,
                     int accumulate, T* Y, int groups) {
    if (l < 1 || l > RS_LMAX) throw std::invalid_argument("stream_block_prod: l must be in [1, 128]");
    if (pc < 0 || m < 1 || m > INT_MAX) throw std::invalid_argument("stream_block_prod: bad shape");
    const int LP = sb_lp(l), RWV = sb_wave_rows(l);
    const int64_t nsl = table_rows(m, l) - 1, ntiles = nsl / NW;
    const int64_t cells = (nsl + 1) * std::max<int64_t>(pc, 1);
    if (cells > ((int64_t)1 << 29)) throw std::invalid_argument("stream_block_prod: the panel's range table would exceed 2 GiB; use narrower panels");
    int* tp = static_cast<int*>(c->scratch(WS_GRAPH, (size_t)cells * sizeof(int)));
    if (pc > 0) {
        hipLaunchKernelGGL(rstream::stream_tile_ptr_kernel, dim3((unsigned)(((nsl + 1) * pc + 255) / 256)), dim3(256), 0, c->stream, cp, ri,
                           pc, nsl, RWV, tp);
        HIPCHK(hipGetLastError());
    }
    const unsigned grid = (unsigned)(groups > 0 ? std::min<int64_t>(groups, ntiles) : ntiles);
    auto* f = LP == 8 ? stream_block_scatter_kernel<T, 8, 1> : LP == 16 ? stream_block_scatter_kernel<T, 16, 1>
              : LP == 32 ? stream_block_scatter_kernel<T, 32, 1> : l <= 64 ? stream_block_scatter_kernel<T, 64, 1>
                                                                           : stream_block_scatter_kernel<T, 64, 2>;
    hipLaunchKernelGGL(f, dim3(grid), dim3(WG), 0, c->stream, ri, ax, (const int*)tp, pc, m, nsl, X, l, accumulate, Y);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" int rcppml_hip_stream_block_geometry(int dtype, int l, int64_t* out) {
    if (!out || l < 1 || l > RS_LMAX || (dtype != RCPPML_F32 && dtype != RCPPML_F64)) {
        rcppml_err() = "stream_block_geometry: l in [1, 128], dtype 0 or 1";
        return 1;
    }
    out[0] = sb_tile_rows(l); out[1] = NW; out[2] = sb_wave_rows(l); out[3] = sb_lp(l);
    out[4] = 4 * NW;            // range-table bytes per (tile, panel column); the table has 4 more per panel column
    return 0;
}

extern "C" int rcppml_hip_stream_block_prod(rcppml_hip_ctx* c, int dtype, const int* col_ptr, const int* row_idx, const void* values,
                                            int64_t nrows, int64_t ncols, int l, const void* X, int accumulate, void* Y, int groups) {
    try {
        HIPCHK(hipSetDevice(c->device));
        if (dtype == RCPPML_F32) block_prod_impl<float>(c, col_ptr, row_idx, (const float*)values, nrows, ncols, l, (const float*)X, accumulate, (float*)Y, groups);
        else block_prod_impl<double>(c, col_ptr, row_idx, (const double*)values, nrows, ncols, l, (const double*)X, accumulate, (double*)Y, groups);
        return 0;
    }
    RCPPML_CATCH_RET
}

namespace {

struct SvdStreamArgs {
    const PanelSource* src;
    int k, l, q, center;
    uint64_t seed;
    std::vector<double> U, V, d, mu;
    int64_t passes = 0, ops = 0;
};

// Engine::randomized of ops_svd.hip with forward() and backward() taken over the panels; orth(), the sketch, the final Gram and
// the l x l stage are the resident engine's kernels and host code, launched as there.
template <class T>
void fit_stream_svd(SvdStreamArgs& P) {
    const PanelSource& S = *P.src;
    const int dt = DT<T>::id, K = P.k, l = P.l, q = P.q;
    const int m = (int)S.m, n = (int)S.n;
    const int64_t np_ = S.panels();
    const int lp = l > 32 ? WAVE : (int)std::max(1.0, std::exp2(std::ceil(std::log2((double)l))));
    const int nbm = (m + RS_RB - 1) / RS_RB, nbn = (n + RS_RB - 1) / RS_RB, np = rs_np(l);
    const double thr = (double)l * (double)std::numeric_limits<T>::epsilon();
    bool aligned = true;                                        // every panel starts on a record block of Z
    for (int64_t pq = 1; pq < np_; ++pq) aligned = aligned && S.pb[pq] % RS_RB == 0;

    CtxGuard g(env_device());
    rcppml_hip_ctx* c = g.c;
    hipStream_t s = g.s;
    PanelBuffer<T> panel(S, c, s);
    DevBuf bY, bZ, bPm, bPn, bRi, bLi, bG, bmu, bones;
    T* Y = dalloc<T>(bY, (size_t)l * m);
    T* Z = dalloc<T>(bZ, (size_t)l * n);
    double* Pm = dalloc<double>(bPm, (size_t)(nbm + 1) * np);
    double* Pn = dalloc<double>(bPn, (size_t)(nbn + 1) * np);
    double* Ri = dalloc<double>(bRi, (size_t)l * l);
    double* Li = dalloc<double>(bLi, (size_t)l * l);
    double* G = dalloc<double>(bG, (size_t)l * l);
    T* mu = nullptr;
    auto* f_omega = RSV_BY_WIDTH(rs_omega_kernel, l);
    auto* f_prod = RSV_BY_WIDTH(rs_prod_kernel, l);
    auto* f_apply = RSV_BY_WIDTH(rs_apply_kernel, l);
    auto* f_finish = RSV_BY_WIDTH(stream_block_finish_kernel, l);
    auto blocks = [](int64_t len) { return dim3((unsigned)((len + WG - 1) / WG)); };
    bool first_visit = true;
    auto visit = [&](int64_t pq) {                              // panel pq resident; one device op (two with the fp32 cast)
        panel.load(pq, first_visit);
        P.ops += 1 + (PanelBuffer<T>::f32 ? 1 : 0);
    };
    auto end_pass = [&] { first_visit = false; ++P.passes; };

    if (P.center) {             // row means: the scatter product at l = 1 against ones, then / n
        mu = dalloc<T>(bmu, (size_t)m);
        T* ones = dalloc<T>(bones, (size_t)S.pc);
        hipLaunchKernelGGL(stream_fill_kernel<T>, blocks(S.pc), dim3(WG), 0, s, ones, S.pc, T(1));
        for (int64_t pq = 0; pq < np_; ++pq) {
            visit(pq);
            OPCHK(rcppml_hip_stream_block_prod(c, dt, panel.cp(), panel.ri(), panel.ax(), m, S.pb[pq + 1] - S.pb[pq], 1, ones, pq > 0, mu, 0));
            ++P.ops;
        }
        hipLaunchKernelGGL(stream_scale_kernel<T>, blocks(m), dim3(WG), 0, s, mu, (int64_t)m, (T)n);
        HIPCHK(hipGetLastError());
        end_pass();
    }
    auto forward = [&] {        // Y = A~ Z: scattered panel by panel, then the centering term and Y's records once
        for (int64_t pq = 0; pq < np_; ++pq) {
            visit(pq);
            OPCHK(rcppml_hip_stream_block_prod(c, dt, panel.cp(), panel.ri(), panel.ax(), m, S.pb[pq + 1] - S.pb[pq], l,
                                               Z + (size_t)S.pb[pq] * l, pq > 0, Y, 0));
            ++P.ops;
        }
        hipLaunchKernelGGL(f_finish, dim3(nbm), dim3(WG), 0, s, Y, (long)m, l, (const double*)Pn, nbn, (const T*)mu, P.center ? 1 : 0, Pm);
        HIPCHK(hipGetLastError());
        ++P.ops;
        end_pass();
    };
    auto backward = [&] {       // Z = A~' Y: rs_prod_kernel on the panel's own column pointers writes the panel's rows of Z
        for (int64_t pq = 0; pq < np_; ++pq) {
            visit(pq);
            const int64_t j0 = S.pb[pq], pc = S.pb[pq + 1] - j0;
            hipLaunchKernelGGL(f_prod, dim3((unsigned)((pc + RS_RB - 1) / RS_RB)), dim3(WG), 0, s, panel.cp(), panel.ri(), panel.ax(), (long)pc,
                               (const T*)Y, l, lp, (const double*)Pm, nbm, (const T*)nullptr, P.center ? 2 : 0, Z + (size_t)j0 * l,
                               Pn + (size_t)(j0 / RS_RB) * np);
            HIPCHK(hipGetLastError());
            ++P.ops;
        }
        if (!aligned) {         // a record block straddles two panels: Z's records are written again, whole
            hipLaunchKernelGGL(f_finish, dim3(nbn), dim3(WG), 0, s, Z, (long)n, l, (const double*)Pm, nbm, (const T*)nullptr, 0, Pn);
            HIPCHK(hipGetLastError());
            ++P.ops;
        }
        end_pass();
    };
    auto orth = [&](T* X, long len, int nb, double* Pr, const T* wt) {
        hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)Pr, nb, l, thr, Ri, Li, G, 0);
        hipLaunchKernelGGL(f_apply, dim3(nb), dim3(WG), 0, s, X, len, l, (const double*)Ri, (const T*)nullptr, 1, Pr);
        hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)Pr, nb, l, thr, Ri, Li, G, 0);
        hipLaunchKernelGGL(f_apply, dim3(nb), dim3(WG), 0, s, X, len, l, (const double*)Ri, wt, 0, Pr);
        HIPCHK(hipGetLastError());
        P.ops += 4;
    };
    hipLaunchKernelGGL(f_omega, dim3(nbn), dim3(WG), 0, s, Z, (long)n, l, (unsigned long long)(P.seed == 0 ? 42ull : P.seed), Pn);
    ++P.ops;
    forward();
    for (int it = 0; it < q; ++it) {
        orth(Y, (long)m, nbm, Pm, mu);
        backward();
        orth(Z, (long)n, nbn, Pn, (const T*)nullptr);
        forward();
    }
    orth(Y, (long)m, nbm, Pm, mu);
    backward();                                                 // Bt, not orthonormalised
    hipLaunchKernelGGL(rs_chol_kernel, dim3(1), dim3(WG), 0, s, (const double*)Pn, nbn, l, thr, Ri, Li, G, 1);
    HIPCHK(hipGetLastError());
    ++P.ops;
    std::vector<double> Gh((size_t)l * l);
    download<double>(Gh.data(), G, Gh.size(), s);
    const int kc = std::min(K, l);
    std::vector<double> wu, wv;
    rs_small_stage(Gh, l, kc, P.d, wu, wv);
    DevBuf dwu, dwv, ou, ov;
    const double* Wu = upload<double>(dwu, wu.data(), wu.size(), s);
    const double* Wv = upload<double>(dwv, wv.data(), wv.size(), s);
    dalloc<T>(ou, (size_t)m * kc); dalloc<T>(ov, (size_t)n * kc);
    hipLaunchKernelGGL(rs_rotate_kernel<T>, dim3((m + NW - 1) / NW), dim3(WG), 0, s, (const T*)Y, (long)m, l, Wu, kc, ou.as<T>());
    hipLaunchKernelGGL(rs_rotate_kernel<T>, dim3((n + NW - 1) / NW), dim3(WG), 0, s, (const T*)Z, (long)n, l, Wv, kc, ov.as<T>());
    HIPCHK(hipGetLastError());
    P.ops += 2;
    P.U.resize((size_t)m * kc);
    P.V.resize((size_t)n * kc);
    download_cast<T>(c, ou, P.U.size(), P.U.data(), s);
    download_cast<T>(c, ov, P.V.size(), P.V.data(), s);
    if (P.center) {
        P.mu.resize((size_t)m);
        download_cast<T>(c, bmu, P.mu.size(), P.mu.data(), s);
    }
}

}  // namespace

extern "C" void rcppml_gpu_svd_streaming_ex(const int* col_ptr, const int* row_idx, const double* values, int* nnz, const char* spz_path,
                                            int* m, int* n, int* k, int* center, int* seed, int* max_iter, int* precision,
                                            int* panel_cols, int* devices, double* U, double* d, double* V, double* out_row_means,
                                            int64_t* out_info, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !n || !k || !center || !seed || !max_iter || !precision || !panel_cols) throw std::invalid_argument("null scalar argument");
        if (!U || !d || !V || !out_info) throw std::invalid_argument("null output");
        if (spz_path && col_ptr) throw std::invalid_argument("data: pass host CSC arrays or an .spz path, not both");
        if (devices && *devices > 1) throw std::invalid_argument("devices > 1: the streamed SVD runs on one device");
        if (*m < 1 || *n < 1) throw std::invalid_argument("m and n must be >= 1");
        if (*precision != RCPPML_F32 && *precision != RCPPML_F64) throw std::invalid_argument("precision must be 0 (fp32) or 1 (fp64)");
        if (*panel_cols < 0) throw std::invalid_argument("panel_cols must be >= 0 (0 = automatic)");
        const int mn = std::min(*m, *n);
        if (*k < 1 || *k > mn) throw std::invalid_argument("k must be in [1, min(m, n)]");
        const int l = *k + std::max(10, *k / 5);
        if (l > RS_LMAX)
            throw std::invalid_argument("k: the sketch dimension l = k + max(10, k / 5) = " + std::to_string(l) + " is above the limit of " +
                                        std::to_string(RS_LMAX));
        if (l > mn)
            throw std::invalid_argument("k: the sketch dimension l = k + max(10, k / 5) = " + std::to_string(l) + " is above min(m, n) = " +
                                        std::to_string(mn));
        if (*center && !out_row_means) throw std::invalid_argument("null output");
        PanelSource src;
        if (spz_path) src.open_spz(spz_path, *m, *n);
        else src.open_csc(col_ptr, row_idx, values, nnz, *m, *n);
        const size_t el = *precision == RCPPML_F32 ? 4 : 8;
        // the widest panel a 2 GiB range table allows, for the l-wide products and for the l = 1 row-mean pass
        const int64_t trows = std::max(table_rows(*m, l), *center ? table_rows(*m, 1) : 0);
        const int64_t cap = std::max<int64_t>(1, ((int64_t)1 << 29) / trows);
        src.plan(*panel_cols, cap);
        if (src.pc > cap)
            throw std::invalid_argument("panel_cols: the range table of the scatter kernel would exceed 2 GiB at " + std::to_string(src.pc) +
                                        " columns per panel; use at most " + std::to_string(cap));
        SvdStreamArgs P{};
        P.src = &src; P.k = *k; P.l = l; P.center = *center != 0; P.seed = (uint64_t)(uint32_t)*seed;
        P.q = *max_iter <= 0 ? 3 : std::min(*max_iter, 10);
        const size_t panel_bytes = src.buffer_bytes(el), table_bytes = (size_t)trows * (size_t)src.pc * 4;
        // the two blocks, the rotated outputs with their fp64 staging, the row means and ones, the records and small matrices; the
        // panel buffer; the range table; .spz: the decoder's scratch
        const size_t M = (size_t)*m, N = (size_t)*n, L = (size_t)l;
        device_ready((M + N) * (L * el + (size_t)*k * (el + 8)) + (M + (size_t)src.pc) * (el + 8) +
                         (M / RS_RB + N / RS_RB + 4) * (size_t)rs_np(l) * 8 + (3 * L * L + 2 * L * (size_t)*k) * 8 + panel_bytes + table_bytes +
                         src.decode_bytes() + ((size_t)64 << 20),
                     "the streamed SVD");
        if (*precision == RCPPML_F32) fit_stream_svd<float>(P);
        else fit_stream_svd<double>(P);
        std::copy(P.U.begin(), P.U.end(), U);
        std::copy(P.V.begin(), P.V.end(), V);
        std::copy(P.d.begin(), P.d.end(), d);
        if (P.center) std::copy(P.mu.begin(), P.mu.end(), out_row_means);
        out_info[0] = P.passes; out_info[1] = src.panels(); out_info[2] = src.pc; out_info[3] = (int64_t)panel_bytes;
        out_info[4] = (int64_t)table_bytes; out_info[5] = P.ops; out_info[6] = P.q; out_info[7] = l;
    });
}
