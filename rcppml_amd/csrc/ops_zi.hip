// ops_zi.hip -- the zero-inflated GP / NB stage on the device (kernels: kernels_zi.hip.h): what the reference's CPU fit runs after
// the dispersion update of every ALS iteration (inst/include/FactorNet/nmf/fit_cpu.hpp:1285-1552) -- zi_em_iters rounds of E-step
// (:1291-1437) and M-step (:1439-1470), each followed by the GP theta floor (:1473-1478), then one soft imputation (:1490-1550).
// The reference has no device path for it (its bridge carries no zi slot), so the CPU fit is the specification.
//
// rcppml_gpu_zi_em_double is the stage alone; rcppml_gpu_nmf_zi_double (plugin.hip) runs it inside the ALS loop through
// rcppml_zi::Stage.  Scope: fp64, sparse (CSC) input, ZI mode ROW or COL, loss GP or NB, dispersion none / global / per row.
// fp32, dense input, masks, cross-validation and several devices are refused.
//
// Repeatability: no floating-point atomics; the z sums are per-tile partials in a fixed order, added in tile order.  The kernels
// walk the tiles with a grid-stride loop, so the result does not depend on the number of workgroups: RCPPML_GPU_ZI_GRID (read
// here only) overrides that number for the tests.
#include "zi_stage.hip.h"
#include "kernels_zi.hip.h"

#include <cmath>
#include <string>
#include <vector>

namespace rcppml_zi {
using namespace rzi;

void validate_common(int loss_type, int zi_mode, int zi_em_iters, int dispersion_mode, int k) {
    if (zi_mode == 3)      // core/config.hpp:437-440
        throw std::invalid_argument("zi_mode=TWOWAY is disabled due to numerical instability on high-sparsity data. Use ZI_ROW or ZI_COL instead.");
    if (zi_mode != 1 && zi_mode != 2) throw std::invalid_argument("zi_mode must be ROW (1) or COL (2)");
    if (loss_type != LOSS_GP && loss_type != LOSS_NB)      // core/config.hpp:441-444
        throw std::invalid_argument("Zero-inflation (zi_mode != NONE) requires GP or NB loss. MSE, Gamma, InvGauss, and Tweedie do not support zero-inflation.");
    if (dispersion_mode == 3)
        throw std::invalid_argument("zero-inflation with dispersion='per_col' is refused: the reference indexes the dispersion vector by row there (fit_cpu.hpp:1333, :1337)");
    if (dispersion_mode < 0 || dispersion_mode > 3) throw std::invalid_argument("bad dispersion mode");
    if (zi_em_iters < 1) throw std::invalid_argument("zi_em_iters must be >= 1");
    if (k < 1 || k > 128) throw std::invalid_argument("zero-inflated losses: k must be in [1, 128]");
}

void validate_csc(const int* col_ptr, const int* row_idx, int64_t m, int64_t n, int64_t nnz) {
    if (!col_ptr || (nnz > 0 && !row_idx)) throw std::invalid_argument("null CSC array");
    check_csc_strict(col_ptr, row_idx, m, n, nnz);
}

size_t stage_bytes(int64_t m, int64_t n, int k, int zi_mode, bool imputed, bool transposed, bool full_index) {
    const size_t M = (size_t)m, N = (size_t)n;
    const size_t ntr = (M + TM - 1) / TM, ntc = (N + TN - 1) / TN;
    size_t b = 8 * ntr * N;                                               // bitmask
    b += 8 * (zi_mode == MODE_ROW ? ntc * M : ntr * N);                   // tile partials
    b += 12 * (zi_mode == MODE_ROW ? M : N) + 8 * std::max(M, N);         // z sums, zero counts, pi
    b += 8 * (size_t)k * M;                                               // a = W_T o d
    if (imputed) b += 8 * M * N;
    if (transposed) b += 8 * M * N;
    if (full_index) b += 2 * 4 * M * N + 4 * (M + N + 2);
    return b;
}

void pi_init_host(const int* col_ptr, const int* row_idx, int64_t m, int64_t n, int zi_mode, std::vector<double>& pi,
                  std::vector<int>& zero_count) {
    if (zi_mode == MODE_ROW) {
        std::vector<int> cnt((size_t)m, 0);
        for (int64_t e = 0; e < col_ptr[n]; ++e) ++cnt[row_idx[e]];
        pi.resize((size_t)m);
        zero_count.resize((size_t)m);
        for (int64_t i = 0; i < m; ++i) {
            const double zero_rate = 1.0 - static_cast<double>(cnt[i]) / n;            // :367-368
            pi[i] = std::min(zero_rate * 0.5, 0.3);
            zero_count[i] = (int)(n - cnt[i]);
        }
    } else {
        pi.resize((size_t)n);
        zero_count.resize((size_t)n);
        for (int64_t j = 0; j < n; ++j) {
            const int c = col_ptr[j + 1] - col_ptr[j];
            const double zero_rate = 1.0 - static_cast<double>(c) / m;                 // :387-388
            pi[j] = std::min(zero_rate * 0.5, 0.3);
            zero_count[j] = (int)(m - c);
        }
    }
}

void Stage::setup(hipStream_t s, int64_t m_, int64_t n_, int k_, int loss_, int mode_, const int* d_col_ptr, const int* d_row_idx,
                  const double* d_values, const std::vector<double>& pi0, const std::vector<int>& zero_count, bool imputed,
                  bool transposed, bool full_index) {
    m = m_; n = n_; k = k_; loss = loss_; mode = mode_;
    ntr = (m + TM - 1) / TM;
    ntc = (n + TN - 1) / TN;
    const int64_t ntiles = ntr * ntc;
    if (ntiles >= ((int64_t)1 << 31)) throw std::invalid_argument("m x n is too large for the tile grid");
    int64_t g = std::min<int64_t>(ntiles, (int64_t)1 << 20);
    if (const char* e = getenv("RCPPML_GPU_ZI_GRID")) {          // test hook: any number of workgroups gives the same bits
        const long long v = atoll(e);
        if (v >= 1) g = std::min<int64_t>(v, ntiles);
    }
    grid = (unsigned)g;
    const size_t words = (size_t)ntr * (size_t)n;
    bits.alloc(words * 8);
    HIPCHK(hipMemsetAsync(bits.p, 0, words * 8, s));
    hipLaunchKernelGGL(bitmask_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, d_col_ptr, d_row_idx, m, n,
                       bits.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    part.alloc(8 * (size_t)(mode == MODE_ROW ? ntc * m : ntr * n));
    zsum.alloc(8 * (size_t)len());
    a.alloc(8 * (size_t)k * (size_t)m);
    zcnt.alloc(4 * (size_t)len());
    pi.alloc(8 * (size_t)len());
    HIPCHK(hipMemcpyAsync(zcnt.p, zero_count.data(), 4 * (size_t)len(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(pi.p, pi0.data(), 8 * (size_t)len(), hipMemcpyHostToDevice, s));
    const size_t mn = (size_t)m * (size_t)n;
    if (imputed) { imp.alloc(8 * mn); HIPCHK(hipMemsetAsync(imp.p, 0, 8 * mn, s)); }
    if (transposed) { impT.alloc(8 * mn); HIPCHK(hipMemsetAsync(impT.p, 0, 8 * mn, s)); }
    if (imputed || transposed) {
        hipLaunchKernelGGL(scatter_stored_kernel, dim3((unsigned)((n + 3) / 4)), dim3(NT), 0, s, d_col_ptr, d_row_idx, d_values, m, n,
                           imputed ? imp.as<double>() : nullptr, transposed ? impT.as<double>() : nullptr);
        HIPCHK(hipGetLastError());
    }
    if (full_index) {
        if (mn >= ((size_t)1 << 31)) throw std::invalid_argument("zero-inflated fit: m * n must be below 2^31 (the dense IRLS half-updates index A_imputed with 32-bit offsets)");
        const unsigned blocks = (unsigned)((mn + 256) / 256);
        fwd_p.alloc(4 * ((size_t)n + 1)); fwd_i.alloc(4 * mn);
        bwd_p.alloc(4 * ((size_t)m + 1)); bwd_i.alloc(4 * mn);
        hipLaunchKernelGGL(full_index_kernel, dim3(blocks), dim3(256), 0, s, (int)m, n, fwd_p.as<int>(), fwd_i.as<int>());
        hipLaunchKernelGGL(full_index_kernel, dim3(blocks), dim3(256), 0, s, (int)n, m, bwd_p.as<int>(), bwd_i.as<int>());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s));          // the host vectors may go out of scope
}

namespace {
template <int LOSS, int MODE>
void launch_pair(bool impute, unsigned grid, hipStream_t s, const ZiArgs& za) {
    if (impute) hipLaunchKernelGGL((zi_impute_kernel<LOSS, MODE>), dim3(grid), dim3(NT), 0, s, za);
    else hipLaunchKernelGGL((zi_estep_kernel<LOSS, MODE>), dim3(grid), dim3(NT), 0, s, za);
}
void launch(bool impute, int loss, int mode, unsigned grid, hipStream_t s, const ZiArgs& za) {
    if (loss == LOSS_NB) {
        if (mode == MODE_ROW) launch_pair<LOSS_NB, MODE_ROW>(impute, grid, s, za);
        else launch_pair<LOSS_NB, MODE_COL>(impute, grid, s, za);
    } else {
        if (mode == MODE_ROW) launch_pair<LOSS_GP, MODE_ROW>(impute, grid, s, za);
        else launch_pair<LOSS_GP, MODE_COL>(impute, grid, s, za);
    }
    HIPCHK(hipGetLastError());
}
}  // namespace

void Stage::run(rcppml_hip_ctx* c, hipStream_t s, const double* W_T, const double* d, const double* H, double* disp, int em_iters,
                double theta_min) {
    OPCHK(rcppml_hip_mul_rows(c, RCPPML_F64, W_T, k, m, d, a.p));          // W_Td_zi = W_T with d applied (:1288-1289)
    ZiArgs za{};
    za.A = a.as<double>(); za.H = H; za.disp = disp; za.pi = pi.as<double>(); za.bits = bits.as<unsigned long long>();
    za.m = m; za.n = n; za.k = k; za.ntr = (int)ntr; za.ntiles = ntr * ntc;
    za.part = part.as<double>(); za.imp = imp.as<double>(); za.impT = impT.as<double>();
    const int64_t L = len();
    const int64_t nparts = mode == MODE_ROW ? ntc : ntr;
    const bool floor_theta = loss == LOSS_GP && theta_min > 0;
    const int64_t mlen = floor_theta ? std::max(L, m) : L;
    for (int it = 0; it < em_iters; ++it) {
        launch(false, loss, mode, grid, s, za);
        hipLaunchKernelGGL(zi_sum_partials_kernel, dim3((unsigned)((L + NT - 1) / NT)), dim3(NT), 0, s, part.as<double>(), nparts, L,
                           zsum.as<double>());
        hipLaunchKernelGGL(zi_mstep_kernel, dim3((unsigned)((mlen + NT - 1) / NT)), dim3(NT), 0, s, zsum.as<double>(), zcnt.as<int>(), L,
                           (double)(mode == MODE_ROW ? n : m), pi.as<double>(), floor_theta ? disp : nullptr, m, theta_min);
        HIPCHK(hipGetLastError());
    }
    if (imp.p || impT.p) launch(true, loss, mode, grid, s, za);
}

}  // namespace rcppml_zi

// The stage alone (fit_cpu.hpp:1285-1552): pi (m for ROW, n for COL) and, for GP with *theta_min > 0, disp (m) are updated in
// place; out_imputed (m x n column-major, may be NULL) receives A_imputed.
extern "C" void rcppml_gpu_zi_em_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz, int* m, int* n,
                                        int* k, const double* W_T, const double* d, const double* H, double* disp, int* loss_type,
                                        int* zi_mode, int* zi_em_iters, double* theta_min, double* pi, double* out_imputed,
                                        int* out_status) {
    using namespace rcppml_zi;
    entry_guard(out_status, [&] {
        if (!m || !n || !k || !nnz || !loss_type || !zi_mode || !zi_em_iters || !theta_min) throw std::invalid_argument("null scalar argument");
        if (*m < 1 || *n < 1) throw std::invalid_argument("m and n must be >= 1");
        validate_common(*loss_type, *zi_mode, *zi_em_iters, 2, *k);
        if (*nnz < 0) throw std::invalid_argument("nnz must be >= 0");
        if (*nnz > 0 && !values) throw std::invalid_argument("null CSC array");
        if (!W_T || !d || !H || !disp || !pi) throw std::invalid_argument("null model array");
        if (!std::isfinite(*theta_min)) throw std::invalid_argument("theta_min must be finite");
        const int64_t M = *m, N = *n, NNZ = *nnz;
        const int K = *k;
        validate_csc(col_ptr, row_idx, M, N, NNZ);
        all_finite(values, (size_t)NNZ, "the matrix");
        all_finite(W_T, (size_t)K * M, "W");
        all_finite(d, (size_t)K, "d");
        all_finite(H, (size_t)K * N, "H");
        all_finite(disp, (size_t)M, "the dispersion vector");
        const int64_t L = *zi_mode == 1 ? M : N;
        all_finite(pi, (size_t)L, "pi");
        for (int64_t q = 0; q < L; ++q)
            if (pi[q] < 0.0 || pi[q] > 1.0) throw std::invalid_argument("pi must lie in [0, 1]");
        const bool want = out_imputed != nullptr;
        device_ready(stage_bytes(M, N, K, *zi_mode, want, false, false) + (size_t)(N + 1) * 4 + (size_t)NNZ * 12 +
                         8 * ((size_t)K * (size_t)(M + N) + K + M) + 65536,
                     "the zero-inflated fit");
        CtxGuard g(env_device());
        hipStream_t s = g.s;
        DevBuf dp, di, dx, dW, dd, dH, ddisp;
        upload_ints(col_ptr, (size_t)N + 1, dp, s);
        if (NNZ > 0) upload_ints(row_idx, (size_t)NNZ, di, s);
        else di.alloc(16);
        upload(dx, values, (size_t)NNZ, s);
        upload(dW, W_T, (size_t)K * M, s);
        upload(dd, d, (size_t)K, s);
        upload(dH, H, (size_t)K * N, s);
        upload(ddisp, disp, (size_t)M, s);
        std::vector<double> pi0;
        std::vector<int> zc;
        pi_init_host(col_ptr, row_idx, M, N, *zi_mode, pi0, zc);
        pi0.assign(pi, pi + L);                                                   // the caller's pi; the counts are the CSC's
        Stage st;
        st.setup(s, M, N, K, *loss_type, *zi_mode, dp.as<int>(), di.as<int>(), dx.as<double>(), pi0, zc, want, false, false);
        st.run(g.c, s, dW.as<double>(), dd.as<double>(), dH.as<double>(), ddisp.as<double>(), *zi_em_iters, *theta_min);
        std::vector<double> hpi((size_t)L), hdisp((size_t)M);
        HIPCHK(hipMemcpyAsync(hpi.data(), st.pi.p, 8 * (size_t)L, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hdisp.data(), ddisp.p, 8 * (size_t)M, hipMemcpyDeviceToHost, s));
        if (want) HIPCHK(hipMemcpyAsync(out_imputed, st.imp.p, 8 * (size_t)M * (size_t)N, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::copy(hpi.begin(), hpi.end(), pi);
        std::copy(hdisp.begin(), hdisp.end(), disp);
    });
}
