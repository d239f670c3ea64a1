// zi_stage.hip.h -- host interface of the zero-inflated GP / NB stage (ops_zi.hip; kernels: kernels_zi.hip.h), shared by the stage's
// own entry (rcppml_gpu_zi_em_double) and the ALS loop of plugin.hip (rcppml_gpu_nmf_zi_double).  fp64, sparse input, mode ROW / COL.
#pragma once
#include "entry_common.hip.h"

namespace rcppml_zi {

// what the caller's arguments must satisfy before anything touches the device; throws std::invalid_argument with the reason
void validate_common(int loss_type, int zi_mode, int zi_em_iters, int dispersion_mode, int k);
// rows strictly increasing within a column (the dgCMatrix invariant: the bitmask build and the scatter rely on it)
void validate_csc(const int* col_ptr, const int* row_idx, int64_t m, int64_t n, int64_t nnz);

// device bytes of the stage's own arrays: the bitmask, the tile partials, the z sums, the zero counts, a = W_T o d, and -- when asked
// for -- A_imputed, A_imputed^T (m n doubles each) and the two full index sets (m n + extent + 1 ints each)
size_t stage_bytes(int64_t m, int64_t n, int k, int zi_mode, bool imputed, bool transposed, bool full_index);

// pi = min(0.5 (1 - stored / extent), 0.3) per row (ROW) or column (COL) and the counts of unstored entries, from the host CSC
// (fit_cpu.hpp:355-400)
void pi_init_host(const int* col_ptr, const int* row_idx, int64_t m, int64_t n, int zi_mode, std::vector<double>& pi,
                  std::vector<int>& zero_count);

struct Stage {
    int64_t m = 0, n = 0, ntr = 0, ntc = 0;
    int k = 0, loss = 0, mode = 0;
    unsigned grid = 1;
    DevBuf bits, part, zsum, zcnt, a, pi, imp, impT, fwd_p, fwd_i, bwd_p, bwd_i;
    int64_t len() const { return mode == 1 ? m : n; }
    // the device CSC (rows strictly increasing within a column), the unstored counts and pi from the host; `imputed` / `transposed`:
    // keep A_imputed / A_imputed^T (stored entries scattered here, once); `full_index`: the index arrays of the CSCs that store every
    // entry of the two (what rcppml_hip_solve_irls takes for the dense IRLS half-updates)
    void setup(hipStream_t s, int64_t m_, int64_t n_, int k_, int loss_, int mode_, const int* d_col_ptr, const int* d_row_idx,
               const double* d_values, const std::vector<double>& pi0, const std::vector<int>& zero_count, bool imputed,
               bool transposed, bool full_index);
    // em_iters x (E-step, M-step, GP theta floor), then one imputation when A_imputed / A_imputed^T are kept.  W_T (k x m), d (k),
    // H (k x n), disp (m; floored in place for GP when theta_min > 0): device, fp64
    void run(rcppml_hip_ctx* c, hipStream_t s, const double* W_T, const double* d, const double* H, double* disp, int em_iters,
             double theta_min);
};

}  // namespace rcppml_zi
