// ops_chol_wide.hip -- blocked MFMA Cholesky + clip for the ranks above the lane-per-column solve (kernels_chol_wide.hip.h);
// reached from solve_chol_impl in ops_solve.hip
#include "common.hip.h"
#include "kernels_chol_wide.hip.h"

using namespace rk;

template <class T, int NBMAX>
static void chol_wide_solve_launch(rcppml_hip_ctx* c, const T* W, const T* LT, const T* invD, const T* invDT, const T* B, T* X,
                                   int k, int nb, int64_t ncols, T l1_pre, int nonneg, T ub_post) {
    const int64_t per_wg = (int64_t)CHOLW_WAVES * CholWide<T>::BS;
    const int64_t nwg = (ncols + per_wg - 1) / per_wg;
    hipLaunchKernelGGL((chol_wide_solve_kernel<T, NBMAX>), dim3((unsigned)nwg), dim3(CHOLW_THREADS), 0, c->stream, W, LT, invD,
                       invDT, B, X, k, nb, ncols, l1_pre, nonneg, ub_post);
    HIPCHK(hipGetLastError());
}

template <class T>
static void chol_wide_impl(rcppml_hip_ctx* c, const T* G, const T* B, T* X, int k, int64_t ncols, T l1_pre, int nonneg,
                           T ub_post) {
    constexpr int BS = CholWide<T>::BS;
    if (k < 1 || k > CHOLW_KMAX) throw std::runtime_error("solve_chol: k out of supported range");
    const int nb = (k + BS - 1) / BS, KP = nb * BS;
    // W | LT | invD | invDT
    T* W = static_cast<T*>(c->scratch(WS_CHOL, (2 * (size_t)KP * KP + 2 * (size_t)nb * BS * BS) * sizeof(T)));
    T* LT = W + (size_t)KP * KP;
    T* invD = LT + (size_t)KP * KP;
    T* invDT = invD + (size_t)nb * BS * BS;
    hipLaunchKernelGGL(chol_wide_factor_kernel<T>, dim3(1), dim3(CHOLW_THREADS), 0, c->stream, G, k, nb, W, LT, invD, invDT);
    HIPCHK(hipGetLastError());
    // the solve's block loops are unrolled to a fixed count (static accumulator registers): 8 blocks, or 16 for fp64 k > 128
    if (nb <= 8) chol_wide_solve_launch<T, 8>(c, W, LT, invD, invDT, B, X, k, nb, ncols, l1_pre, nonneg, ub_post);
    else if constexpr (BS == 16) chol_wide_solve_launch<T, 16>(c, W, LT, invD, invDT, B, X, k, nb, ncols, l1_pre, nonneg, ub_post);
}

void rcppml_solve_chol_wide_f32(rcppml_hip_ctx* c, const float* G, const float* B, float* X, int k, int64_t ncols, float l1_pre,
                                int nonneg, float ub_post) {
    chol_wide_impl<float>(c, G, B, X, k, ncols, l1_pre, nonneg, ub_post);
}
void rcppml_solve_chol_wide_f64(rcppml_hip_ctx* c, const double* G, const double* B, double* X, int k, int64_t ncols,
                                double l1_pre, int nonneg, double ub_post) {
    chol_wide_impl<double>(c, G, B, X, k, ncols, l1_pre, nonneg, ub_post);
}
