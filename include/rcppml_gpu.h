/* ============================================================================
 * rcppml_gpu.h -- C ABI of RcppML_gpu.so, the MI355X (gfx950) backend for RcppML's
 * alternating-NNLS NMF hot path.
 *
 * Two layers, both plain C (pointers and sizes only; no torch / Rcpp / Eigen types):
 *
 *  (1) PLUGIN BOUNDARY -- host-pointer entry points the unmodified R package binds:
 *      R `.C()` through `.gpu_call` (reference R/gpu_backend.R:24-27) and C++
 *      `dlsym(RTLD_DEFAULT, name)` from RcppML.so (reference
 *      inst/include/FactorNet/gpu/loader.hpp:44-48).  Signatures are byte-for-byte the
 *      reference plugin's (src/gpu_bridge_cluster.cu:24-46, src/gpu_bridge_nmf.cu:34-80,
 *      type inst/include/FactorNet/gpu/bridge_nmf.hpp:39-75).  Every scalar is a pointer
 *      (R `.C` convention).  Nothing throws across the boundary: failures set
 *      *out_status = -1 (reference src/gpu_bridge_nmf.cu:206-209), which makes the caller
 *      fall back to its CPU path (inst/include/FactorNet/nmf/fit.hpp:125-133).
 *
 *  (2) DEVICE-LEVEL OPS -- the kernels of the path on caller-owned DEVICE memory and a
 *      caller-supplied HIP stream.  This is what the host harness (the Python modules under rcppml_amd/, one
 *      process per GPU under torch.distributed/RCCL) and bench.py drive; PyTorch only
 *      provides the allocations, the stream and the collectives.
 *
 * All dense matrices are column-major with the factor rank k as leading dimension:
 *   W_T : k x m   (reference "W" in/out array of the ABI, W[f + i*k])
 *   H   : k x n
 *   G   : k x k
 * Sparse input is CSC with int32 indices (dgCMatrix / Eigen::SparseMatrix<_,ColMajor,int>).
 * ==========================================================================*/
#ifndef RCPPML_GPU_H
#define RCPPML_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCPPML_GPU_API __attribute__((visibility("default")))

/* --------------------------------------------------------------------------
 * (1) Plugin boundary
 * ------------------------------------------------------------------------*/

/* Replaces reference src/gpu_bridge_cluster.cu:24-46 (callers: R/gpu_backend.R:101-106,
 * gpu/loader.hpp:73-92 -- arrays of length *max_gpus, normally 8).
 * out_status = 0 and num_gpus > 0  <=>  backend available. */
RCPPML_GPU_API void rcppml_gpu_detect(int* num_gpus, double* total_mem_mb, double* free_mem_mb,
                                      int* max_gpus, int* out_status);

/* Replaces reference src/gpu_bridge_nmf.cu:460-624 (`rcppml_gpu_nmf_unified_float`, the symbol
 * gpu/bridge_nmf.hpp:187 resolves) and :34-210 (`_double`).  73 pointer arguments, order per
 * SURVEY.md Appendix B.  `_float` computes in fp32 (like the reference; set env
 * RCPPML_GPU_PRECISION=fp64 to force fp64), `_double` computes in fp64.  Arrays at the ABI are
 * always double.  W (k x m), H (k x n), d (k) are in/out.  Unlike the reference plugin this one
 * sorts factors by descending d before returning (what CPU nmf() returns) unless env
 * RCPPML_GPU_SORT=0.  Implemented: losses MSE / NB / GP(KL) / Gamma / inverse Gaussian / Tweedie with
 * dispersion none, global or per-row and the robust (Huber) modifier; L1, L2, L21, angular, graph
 * Laplacians, upper bounds, nonneg, projective and symmetric NMF (MSE path); CD and Cholesky+clip;
 * env RCPPML_GPU_DEVICES=n shards plain MSE fits over n devices (plugin_multi.hip).  Not implemented
 * -- REJECTED with *out_status = -1 so the caller falls back to CPU rather than silently dropping
 * them: classifier guides, dispersion = per_col (n values: the bridge's out_theta holds m, gpu/bridge_nmf.hpp:284 --
 * rcppml_gpu_nmf_ex takes a capacity), k > 256 (k > 128 for IRLS losses,
 * explicit masks, angular and graph penalties).  Target regularisation and zero-inflation (zi_mode, zi_em_iters) have no slot in
 * these 73 arguments: see rcppml_gpu_nmf_target and rcppml_gpu_nmf_zi_double below -- through the 73-pointer entries a fit is never
 * zero-inflated. */
#define RCPPML_NMF_UNIFIED_ARGS                                                                    \
    const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz, int* k, \
        double* W, double* H, double* d, int* max_iter, double* tol, double* L1_H, double* L1_W,   \
        double* L2_H, double* L2_W, double* L21_H, double* L21_W, double* ortho_H, double* ortho_W, \
        double* ub_H, double* ub_W, int* cd_maxit, int* verbose, int* seed, int* loss_every,       \
        int* patience, int* nonneg_W, int* nonneg_H, int* loss_type, double* huber_delta,          \
        int* irls_max_iter, double* irls_tol, int* norm_type, int* projective, int* symmetric,     \
        int* solver_mode, const int* graph_W_p, const int* graph_W_i, const double* graph_W_x,     \
        int* graph_W_dim, int* graph_W_nnz, double* graph_W_lambda, const int* graph_H_p,          \
        const int* graph_H_i, const double* graph_H_x, int* graph_H_dim, int* graph_H_nnz,         \
        double* graph_H_lambda, int* gp_dispersion_mode, double* gp_theta_init,                    \
        double* gp_theta_max, double* gp_theta_min, double* nb_size_init, double* nb_size_max,     \
        double* nb_size_min, double* gamma_phi_init, double* gamma_phi_max, double* gamma_phi_min, \
        double* robust_delta, double* tweedie_power, double* out_theta, int* out_theta_len,        \
        const int* guide_H_labels_flat, const int* guide_H_ns, const double* guide_H_lambdas,      \
        const int* guide_H_ncs, int* guide_H_count, int* out_iter, int* out_converged,             \
        double* out_loss, int* out_status, double* out_tol

/* StreamPress / SparsePress v2 `.spz` reader.  Replaces reference `rcppml_sp_read_gpu` /
 * `rcppml_sp_free_gpu` (src/sp_gpu_bridge.cu:41-123, :132-155; bound by R/sp_gpu.R through .C()): reads the file,
 * entropy-decodes it ON THE DEVICE (one wavefront per rANS stream) and returns device pointers to int32 col_ptr (n+1),
 * int32 row_idx (nnz) and double values (nnz) -- the arrays rcppml_gpu_nmf_zerocopy_double takes -- with the addresses
 * stored in doubles (R has no 64-bit integer).  out_status: 0 ok, 1 cannot open, 2 short read, 3 file too small,
 * 4 not a v2 file, 5 decode error.  Row-sorted files: the stored row permutation is applied as the reference decoder applies it.
 * The caller releases the three arrays with rcppml_sp_free_gpu, which also zeroes the addresses. */
RCPPML_GPU_API void rcppml_sp_read_gpu(const char** path_ptr, int* device_id, double* out_col_ptr_addr,
                                       double* out_row_idx_addr, double* out_values_addr, int* out_m, int* out_n,
                                       double* out_nnz, int* out_status);
RCPPML_GPU_API void rcppml_sp_free_gpu(double* col_ptr_addr, double* row_idx_addr, double* values_addr, int* out_status);
/* Zero-copy NMF on a device-resident CSC.  Replaces reference `rcppml_gpu_nmf_zerocopy_double`
 * (src/gpu_bridge_nmf.cu:879-967, called from R/sp_gpu.R through .C()): col_ptr (int32), row_idx (int32) and values
 * (double) are DEVICE pointers whose addresses are passed as doubles (R has no 64-bit integer); W (k x m), H (k x n), d are
 * host buffers, in/out.  MSE loss, CD solver (the entry carries no solver argument), L1 / L2 / L21 / angular / bounds.
 * No upload of A: only the transpose, the factors and the per-iteration loss touch PCIe. */
RCPPML_GPU_API void rcppml_gpu_nmf_zerocopy_double(double* d_col_ptr_addr, double* d_row_idx_addr, double* d_values_addr,
                                                   int* m, int* n, double* nnz_d, int* k, double* W, double* H, double* d,
                                                   int* max_iter, double* tol, double* L1_H, double* L1_W, double* L2_H,
                                                   double* L2_W, double* L21_H, double* L21_W, double* ortho_H,
                                                   double* ortho_W, double* ub_H, double* ub_W, int* cd_maxit, int* verbose,
                                                   int* seed, int* loss_every, int* patience, int* nonneg_W, int* nonneg_H,
                                                   int* loss_type, double* huber_delta, int* irls_max_iter, double* irls_tol,
                                                   int* norm_type, int* out_iter, int* out_converged, double* out_loss,
                                                   int* out_status, double* out_tol);

/* Cross-validation NMF.  Replaces reference `rcppml_gpu_nmf_cv_unified_float` (type
 * inst/include/FactorNet/gpu/bridge_nmf.hpp:77-99, resolved and called at :407-497 by bridge_nmf_cv_sparse): 51 pointer
 * arguments, W (k x m) and H (k x n) are initialised by the caller, d = 1.  Implemented: MSE loss and loss_type 4..8 (GP, NB,
 * Gamma, inverse Gaussian, Tweedie: per-column weighted Grams, nmf/fit_cv.hpp:446-456, 670-689; dispersion settings = the
 * reference's config defaults, the boundary has no slot for them -- rcppml_gpu_nmf_cv_irls_ex below carries them), CD and
 * Cholesky+clip, L1 / L2, both mask_zeros settings, k <= 128; anything else sets out_status = -1 (CPU fallback).  The held-out set is
 * the speckled mask of rcppml_hip_solve_cv with cv_seed, or seed when cv_seed = 0 (core/config.hpp:415-418).  Early
 * stopping: cv_patience = NMF_PATIENCE = 5 (not transmitted by the bridge; RCPPML_GPU_CV_PATIENCE overrides).  On
 * return H carries d and d is returned too (nmf/fit_cv.hpp:1636-1647). */
#define RCPPML_NMF_CV_ARGS                                                                         \
    const int *col_ptr, const int *row_idx, const double *values, int *m, int *n, int *nnz, int *k, \
        double *W, double *H, double *d, int *max_iter, double *tol, double *L1_H, double *L1_W,    \
        double *L2_H, double *L2_W, int *cd_maxit, int *verbose,                                    \
        int *seed_only_used_for_cv_seed_fallback, double *holdout_frac, int *cv_seed,               \
        int *mask_zeros, int *nonneg_W, int *nonneg_H, int *norm_type, int *loss_type,              \
        double *huber_delta, int *irls_max_iter, double *irls_tol, const int *graph_W_p,            \
        const int *graph_W_i, const double *graph_W_x, int *graph_W_dim, int *graph_W_nnz,          \
        double *graph_W_lambda, const int *graph_H_p, const int *graph_H_i,                         \
        const double *graph_H_x, int *graph_H_dim, int *graph_H_nnz, double *graph_H_lambda,        \
        int *projective, int *symmetric, int *solver_mode, int *out_iter, int *out_converged,       \
        double *out_train_loss, double *out_test_loss, double *out_best_test, int *out_best_iter,   \
        int *out_status
RCPPML_GPU_API void rcppml_gpu_nmf_cv_unified_float(RCPPML_NMF_CV_ARGS);
RCPPML_GPU_API void rcppml_gpu_nmf_cv_unified_double(RCPPML_NMF_CV_ARGS);
/* Build-defined: + sort flag, precision (RCPPML_F32/F64), cv_patience, train / test loss histories (may be NULL). */
RCPPML_GPU_API void rcppml_gpu_nmf_cv_ex(RCPPML_NMF_CV_ARGS, int* sort_model, int* precision, int* cv_patience,
                                         double* train_history, double* test_history);
/* CV with the IRLS losses (loss_type 4 GP, 5 NB, 6 Gamma, 7 inverse Gaussian, 8 Tweedie; reference nmf/fit_cv.hpp:446-456, :670-689,
 * :866-961, :1377-1443, nmf/cv_detail.hpp:101-292) runs through ALL the CV entries above.  The reference boundary carries loss_type,
 * irls_max_iter and irls_tol only, so its entries take the reference's config defaults for the rest (per-row GP dispersion with
 * theta_init 0.1 / theta_max 5, Tweedie power 1.5, no robust modifier: core/config.hpp:151-172, math/loss.hpp:109-115); this
 * build-defined entry passes them, and returns GP's theta (out_theta: m doubles, may be NULL). */
RCPPML_GPU_API void rcppml_gpu_nmf_cv_irls_ex(RCPPML_NMF_CV_ARGS, int* sort_model, int* precision, int* cv_patience,
                                              double* train_history, double* test_history, int* dispersion_mode,
                                              double* gp_theta_init, double* gp_theta_max, double* tweedie_power,
                                              double* robust_delta, double* out_theta);

/* Build-defined: rcppml_gpu_nmf_cv_irls_ex + a user mask -- pattern CSC of the m x n mask (mask_p: n + 1, mask_i: *mask_nnz rows, ascending
 * inside a column; NULL / 0 = no mask).  The reference's nmf_fit_cv honours NMFConfig::mask (nmf/fit_cv.hpp:327-331, :491-501, :779-790;
 * nmf/cv_detail.hpp:433-505): a masked entry is in no training sum, its row joins the rows taken out of the column's Gram, and both
 * losses skip it -- computed explicitly per element for MSE too (:1377-1443).  Its CV boundary has no slot for the mask
 * (gpu/bridge_nmf.hpp:77-99), hence this entry. */
RCPPML_GPU_API void rcppml_gpu_nmf_cv_masked_ex(RCPPML_NMF_CV_ARGS, int* sort_model, int* precision, int* cv_patience,
                                                double* train_history, double* test_history, int* dispersion_mode,
                                                double* gp_theta_init, double* gp_theta_max, double* tweedie_power,
                                                double* robust_delta, double* out_theta, const int* mask_p, const int* mask_i,
                                                int* mask_nnz);

/* Dense-input NMF.  Replaces reference `rcppml_gpu_nmf_dense_unified_float` (resolved by
 * inst/include/FactorNet/gpu/bridge_nmf.hpp:544-545; 50 pointers, typedef :101-126): A_data is the m x n column-major
 * matrix as doubles on the host; W (k x m), H (k x n), d in/out as in the sparse entry.  Semantics: the reference's
 * STANDARD path (separate RHS -> features -> nnls_batch / cholesky_clip_batch, nmf/fit_cpu.hpp:540-631, :774-881) --
 * zero start at iteration 0, residual-corrected warm start afterwards -- MSE loss; L1, L2, L21, angular, bounds,
 * projective, symmetric.  loss_type 4..8 and robust_delta > 0 (round 5): the dense IRLS half-updates
 * (nnls_batch_irls_dense, nmf/fit_cpu.hpp:607-614, :855-863 -- EVERY entry weighted, zeros included, each batch from zero),
 * the dense branches of the dispersion updates and explicit_loss_dense; CD solver, k <= 128, m * n < 2^31, no L21 / angular /
 * projective / symmetric; gamma_phi_* take the config defaults (no slot); out_theta holds max(m, n) doubles
 * (gpu/bridge_nmf.hpp:622), *out_theta_len = m, or n under dispersion mode 3.  `_double` is build-defined (fp64 compute). */
#define RCPPML_NMF_DENSE_ARGS                                                                       \
    const double* A_data, int* m, int* n, int* k, double* W, double* H, double* d, int* max_iter,   \
        double* tol, double* L1_H, double* L1_W, double* L2_H, double* L2_W, double* L21_H,         \
        double* L21_W, double* ortho_H, double* ortho_W, double* ub_H, double* ub_W, int* cd_maxit, \
        int* verbose, int* seed, int* loss_every, int* patience, int* nonneg_W, int* nonneg_H,      \
        int* loss_type, double* huber_delta, int* irls_max_iter, double* irls_tol, int* norm_type,  \
        int* gp_dispersion_mode, double* gp_theta_init, double* gp_theta_max, double* gp_theta_min, \
        double* nb_size_init, double* nb_size_max, double* nb_size_min, double* robust_delta,       \
        double* tweedie_power, int* projective, int* symmetric, int* solver_mode, double* out_theta,\
        int* out_theta_len, int* out_iter, int* out_converged, double* out_loss, int* out_status,   \
        double* out_tol
RCPPML_GPU_API void rcppml_gpu_nmf_dense_unified_float(RCPPML_NMF_DENSE_ARGS);
RCPPML_GPU_API void rcppml_gpu_nmf_dense_unified_double(RCPPML_NMF_DENSE_ARGS);

RCPPML_GPU_API void rcppml_gpu_nmf_unified_float(RCPPML_NMF_UNIFIED_ARGS);
RCPPML_GPU_API void rcppml_gpu_nmf_unified_double(RCPPML_NMF_UNIFIED_ARGS);

/* Build-defined extras (not in the reference ABI).  Same 73 arguments plus what the
 * reference bridge does not transmit (gpu/bridge_nmf.hpp:180-346 drops config.mask, cd_tol,
 * sort_model): an explicit mask in CSC (nonzero = masked; nmf/masked_nnls.hpp), cd_tol, sort flag,
 * compute precision (0 = fp32, 1 = fp64) and an optional per-iteration loss history buffer
 * (length >= *max_iter, may be NULL).
 * out_theta CAPACITY: in this entry and in rcppml_gpu_nmf_target, *out_theta_len is read ON INPUT as the number of doubles
 * out_theta can hold (<= 0: m, the reference bridge's buffer, gpu/bridge_nmf.hpp:284); on return it is the number written.
 * dispersion mode 3 (per_col) writes n values and is refused with *out_status = -1 when the capacity is smaller than n. */
RCPPML_GPU_API void rcppml_gpu_nmf_ex(RCPPML_NMF_UNIFIED_ARGS, const int* mask_p, const int* mask_i,
                                      int* mask_nnz, double* cd_tol, int* sort_model,
                                      int* precision, double* loss_history);

/* rcppml_gpu_nmf_ex plus TARGET regularisation (nmf/variant_helpers.hpp:107-146, not carried by the
 * 73-pointer ABI): target_H (k x n) / target_W (k x m) column-major with k leading, NULL = none, and their lambdas.
 *   lambda > 0  enrichment: G.diagonal() += lambda, B += lambda * target;
 *   lambda < 0  PROJ_ADV:   G -= |lambda| * (trace G / trace TG) * TG with TG = target target^T / ncols (nmf/fit.hpp:259-271),
 *               then the eigenvalues of G below 1e-8 are raised to 1e-8 (B untouched).
 * As in the reference (fit_cpu.hpp:430-433) a fit with a target runs the STANDARD path: B materialised, features on
 * (G, B), nnls_batch from zero at iteration 0 and residual-corrected afterwards.  Plain MSE fits only. */
RCPPML_GPU_API void rcppml_gpu_nmf_target(RCPPML_NMF_UNIFIED_ARGS, const int* mask_p, const int* mask_i,
                                          int* mask_nnz, double* cd_tol, int* sort_model, int* precision,
                                          double* loss_history, const double* target_H, double* target_lambda_H,
                                          const double* target_W, double* target_lambda_W);

/* fp64 projection h = NNLS(w^T w, w^T A): GPU entry for R nnls()/predict(), which have no GPU
 * hook in the reference (src/RcppFunctions_utils.cpp:313-366 c_nnls, :23-52 Rcpp_predict).
 * w_T: k x m, A: m x n CSC (host pointers), h: k x n in/out (warm start if *warm != 0). */
RCPPML_GPU_API void rcppml_gpu_nnls_double(const int* col_ptr, const int* row_idx,
                                           const double* values, int* m, int* n, int* nnz, int* k,
                                           const double* w_T, double* h, int* cd_maxit,
                                           double* cd_tol, double* L1, double* L2, double* ub,
                                           int* nonneg, int* warm, int* out_status);

/* fp64 evaluate(): mean squared error of W diag(d) H against A over all m*n entries or (mask_zeros)
 * over nonzeros only, WITHOUT densifying W H (reference src/RcppFunctions_utils.cpp:95-163 builds
 * the dense m x n product).  W_T: k x m. */
RCPPML_GPU_API void rcppml_gpu_evaluate_mse_double(const int* col_ptr, const int* row_idx,
                                                   const double* values, int* m, int* n, int* nnz,
                                                   int* k, const double* W_T, const double* d,
                                                   const double* H, int* mask_zeros,
                                                   double* out_loss, int* out_status);

/* Per-phase profile of the batch-CD ALS iteration -- the reference's `rcppml_gpu_nmf_profile_double`
 * (src/gpu_bridge_utils.cu:48-57: the same fifteen pointers, in order; :14-36 the slots).  fp64; W_T and H from
 * SplitMix64(*seed) (one stream, W_T first: initialize_factors), d = 1; one untimed warm-up iteration, then up to *max_iter
 * iterations with a HIP-event pair around every phase and `|prev - loss| / (|prev| + 1e-15) < *tol` from the second timed
 * iteration on; every solve runs *cd_maxit sweeps (no tolerance stop), cold solves start from max(B, 0).
 * out_phase_ms_total[11] / out_phase_ms_per_iter[11] (total / *out_n_iters), slots:
 *   0 gram_H   1 rhs_H   2 nnls_H   3 norm_H   4 gram_W   5 rhs_W by the plan-free gather kernel (the reference's slot holds
 *   its atomicAdd baseline; it is not used by the solve here either)   6 rhs_W planned   7 nnls_W   8 norm_W   9 loss   10 iteration.
 * *out_status 0 / -1 (rcppml_gpu_last_error). */
RCPPML_GPU_API void rcppml_gpu_nmf_profile_double(const int* col_ptr, const int* row_idx, const double* values,
                                                  int* m, int* n, int* nnz, int* k, int* max_iter, double* tol,
                                                  int* cd_maxit, int* seed, double* out_phase_ms_total,
                                                  double* out_phase_ms_per_iter, int* out_n_iters, int* out_status);

/* Clustering (rcppml_amd/csrc/ops_cluster.hip): bipartition() and dclust() with the reference's CPU semantics
 * (inst/include/FactorNet/clustering/bipartition.hpp, dclust.hpp) -- SplitMix64(seed) start (seed 0 -> 12345), the same seed for
 * every split, closed-form rank-2 ALS, 1 - Pearson(w, w_prev) tolerance -- in fp64, all splits of one tree level batched.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), outputs untouched: no device, a malformed CSC, *max_iter < 1 (the CPU
 * reads an uninitialised h), *tol >= 1 or NaN (the CPU runs no iteration), *min_samples < 1 (the CPU never terminates), a seed
 * outside [0, 2^32).  Env RCPPML_GPU_CLUSTER_BUDGET (bytes, default 2 GiB): per-cluster device memory (32 m bytes a split) of one
 * launch batch; a level over it runs in chunks, with the same result.
 *
 * rcppml_gpu_bipartition_double: the reference plugin's 15 pointers (src/gpu_bridge_cluster.cu:57-62) with the buffers R allocates
 * (R/bipartition.R:105-108): partition n ints (0 = samples1, i.e. v > 0; 1 = samples2), v m doubles (the first min(m, n) sample
 * scores are written, nothing past m), center 2 m doubles (center1 then center2), dist 1.  All columns, calc_dist on. */
RCPPML_GPU_API void rcppml_gpu_bipartition_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n,
                                                  int* nnz, int* max_iter, double* tol, int* nonneg, double* seed, int* partition,
                                                  double* v, double* center, double* dist, int* out_status);
/* rcppml_gpu_dclust_double: the reference plugin's 16 pointers (src/gpu_bridge_cluster.cu:105-110).  assignments (n ints): the
 * sample's cluster as its index in the CPU's emission order; *max_clusters > 0 keeps the first *max_clusters clusters and gives
 * the samples of the others -1.  *out_num_clusters: clusters reported. */
RCPPML_GPU_API void rcppml_gpu_dclust_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n,
                                             int* nnz, int* max_clusters, int* min_samples, double* min_dist, int* max_iter,
                                             double* tol, int* nonneg, double* seed, int* assignments, int* out_num_clusters,
                                             int* out_status);
/* Build-defined forms (the Python surface).  Every *_len / *_cap is the buffer's capacity on input and the count written on
 * output; a capacity below what the call needs is refused (status -1) with the size needed in it, nothing else written.
 * rcppml_gpu_bipartition_ex: samples (0-based, any order, duplicates allowed; NULL or *n_samples = 0: all columns), calc_dist
 * switch.  partition / v: one entry per sample (*partition_len, *v_len >= n_samples); center: 2 m (zeros without calc_dist);
 * out_dist -1 without calc_dist; out_iter = ALS iterations run. */
RCPPML_GPU_API void rcppml_gpu_bipartition_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                              const int* samples, int* n_samples, int* max_iter, double* tol, int* nonneg, double* seed,
                                              int* calc_dist, int* partition, int* partition_len, double* v, int* v_len, double* center,
                                              int* center_len, int* out_size1, int* out_size2, double* out_dist, int* out_iter,
                                              int* out_status);
/* rcppml_gpu_dclust_ex: assignments (n ints, emission-order cluster index); per cluster (capacity *cluster_cap): out_size,
 * out_radius (the rejected split's dist with min_dist > 0, else 0), out_node (its node in the split tree), out_center (m doubles
 * per cluster, may be NULL: then not computed).  The split tree (capacity *node_cap): node 0 is the root (parent -1, bit -1),
 * every accepted split adds its two children (bit 0 = samples1, 1 = samples2); node_iter = ALS iterations of the node's
 * bipartition (-1: none was attempted).  A cluster's id is the bits on its path from the root -- any depth. */
RCPPML_GPU_API void rcppml_gpu_dclust_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
                                         int* min_samples, double* min_dist, int* max_iter, double* tol, int* nonneg, double* seed,
                                         int* assignments, int* cluster_cap, int* out_size, double* out_radius, int* out_node,
                                         double* out_center, int* node_cap, int* node_parent, int* node_bit, int* node_iter,
                                         int* out_status);

/* Truncated SVD / PCA (rcppml_amd/csrc/ops_svd.hip): the reference plugin's four entries with its pointer lists
 * (src/gpu_bridge_svd.cu:53, 220, 392, 555) -- 61 pointers for the sparse CSC forms, 58 for the column-major dense forms.  The
 * _float forms take doubles, compute in fp32 on the device and write doubles back.  Outputs in the R wrapper's layout
 * (R/gpu_backend.R:295-420): U m x k_max and V n x k_max column-major with the first *out_k_selected columns written, d, out_iters_per_
 * factor (deflation: one count per factor; Lanczos: the number of steps in entry 0), out_frobenius_norm_sq (of the centered matrix
 * when *center), out_row_means (m, when *center), out_wall_time_ms.  out_test_loss is not written.
 *   *algorithm 0: deflation, the reference's CPU deflation_svd (svd/deflation.hpp:600-915) restated.
 *   *algorithm 1-4 (irlba, lanczos, randomized, krylov) without element constraints: Golub-Kahan-Lanczos with full two-pass
 *     reorthogonalisation (svd/lanczos.hpp); with *k_max = min(m, n) it may take min(m, n) steps instead of min(m, n) - 1.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), outputs untouched: *test_fraction > 0, an obs_mask, a graph with lambda > 0,
 * L21, angular, *robust_delta > 0, element constraints (L1 / L2 / nonneg / upper bound) with *algorithm != 0, *k_max outside
 * [1, min(m, n)], *algorithm outside [0, 4], deflation with *max_iter < 1, a malformed CSC, no device. */
RCPPML_GPU_API void rcppml_gpu_svd_pca_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* k_max, double* U, double* d, double* V, double* tol, int* max_iter,
        int* center, int* verbose, int* seed, int* threads, double* L1_u, double* L1_v, double* L2_u, double* L2_v, int* nonneg_u,
        int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        double* test_fraction, int* cv_seed, int* patience, int* mask_zeros, int* algorithm, const int* graph_u_p,
        const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz, double* graph_u_lambda_val,
        const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim, int* graph_v_nnz,
        double* graph_v_lambda_val, const int* obs_mask_p, const int* obs_mask_i, const double* obs_mask_x, int* obs_mask_rows,
        int* obs_mask_cols, int* obs_mask_nnz, int* out_k_selected, double* out_wall_time_ms, double* out_test_loss,
        int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means, double* robust_delta, int* irls_max_iter,
        double* irls_tol, int* out_status);
RCPPML_GPU_API void rcppml_gpu_svd_pca_float(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* k_max, double* U, double* d, double* V, double* tol, int* max_iter,
        int* center, int* verbose, int* seed, int* threads, double* L1_u, double* L1_v, double* L2_u, double* L2_v, int* nonneg_u,
        int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        double* test_fraction, int* cv_seed, int* patience, int* mask_zeros, int* algorithm, const int* graph_u_p,
        const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz, double* graph_u_lambda_val,
        const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim, int* graph_v_nnz,
        double* graph_v_lambda_val, const int* obs_mask_p, const int* obs_mask_i, const double* obs_mask_x, int* obs_mask_rows,
        int* obs_mask_cols, int* obs_mask_nnz, int* out_k_selected, double* out_wall_time_ms, double* out_test_loss,
        int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means, double* robust_delta, int* irls_max_iter,
        double* irls_tol, int* out_status);
RCPPML_GPU_API void rcppml_gpu_svd_pca_dense_double(const double* A_data, int* m, int* n,
        int* k_max, double* U, double* d, double* V, double* tol, int* max_iter,
        int* center, int* verbose, int* seed, int* threads, double* L1_u, double* L1_v, double* L2_u, double* L2_v, int* nonneg_u,
        int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        double* test_fraction, int* cv_seed, int* patience, int* mask_zeros, int* algorithm, const int* graph_u_p,
        const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz, double* graph_u_lambda_val,
        const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim, int* graph_v_nnz,
        double* graph_v_lambda_val, const int* obs_mask_p, const int* obs_mask_i, const double* obs_mask_x, int* obs_mask_rows,
        int* obs_mask_cols, int* obs_mask_nnz, int* out_k_selected, double* out_wall_time_ms, double* out_test_loss,
        int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means, double* robust_delta, int* irls_max_iter,
        double* irls_tol, int* out_status);
RCPPML_GPU_API void rcppml_gpu_svd_pca_dense_float(const double* A_data, int* m, int* n,
        int* k_max, double* U, double* d, double* V, double* tol, int* max_iter,
        int* center, int* verbose, int* seed, int* threads, double* L1_u, double* L1_v, double* L2_u, double* L2_v, int* nonneg_u,
        int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        double* test_fraction, int* cv_seed, int* patience, int* mask_zeros, int* algorithm, const int* graph_u_p,
        const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz, double* graph_u_lambda_val,
        const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim, int* graph_v_nnz,
        double* graph_v_lambda_val, const int* obs_mask_p, const int* obs_mask_i, const double* obs_mask_x, int* obs_mask_rows,
        int* obs_mask_cols, int* obs_mask_nnz, int* out_k_selected, double* out_wall_time_ms, double* out_test_loss,
        int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means, double* robust_delta, int* irls_max_iter,
        double* irls_tol, int* out_status);

/* Cross-validated / auto-rank and obs-masked deflation SVD (rcppml_amd/csrc/ops_svd.hip, kernels_svd_cv.hip.h).  BUILD-DEFINED: the
 * reference has no such symbols; it runs this inside its deflation loop (svd/deflation.hpp:431-565, :713-781, :869-896), which the four
 * entries above still refuse.  The reference's CPU path is what is restated, not its GPU variant (svd/deflation_gpu.cuh:857-1345, whose
 * hold-out rule differs):
 *   mask      entry (i, j) is held out when SplitMix64::hash(seed, i, j) < UINT64_MAX / inv_prob (rng/rng.hpp:129-170), inv_prob =
 *             (uint64)(1.0 / *test_fraction) (nmf/speckled_cv.hpp:121, taken from the double in both precisions), seed = *cv_seed != 0 ?
 *             *cv_seed : (*seed != 0 ? *seed ^ 0xBEEF : 42) (core/svd_config.hpp:149-151)
 *   test set  sparse: the held-out stored entries, with either *mask_zeros (svd/test_entries.hpp:84-108); dense: every held-out
 *             (i, j) (:131-141); taken from the original A, minus the row mean when *center, in column-major order
 *   training  the pattern of A with held-out values and the values at obs_mask positions set to 0 (:264-315, deflation.hpp:452-487);
 *             both products read it; row means and out_frobenius_norm_sq come from the full A (deflation.hpp:377-417)
 *   updates   |u_hat|^2 and |v|^2 are scaled by 1 - *test_fraction * nnz / (m n) with *mask_zeros, else by 1 - *test_fraction (dense:
 *             1 - *test_fraction either way), where they divide the update and where the element constraints take them
 *             (deflation.hpp:552-559, :724-739, :769-784); not in the warm start or the Rayleigh quotient
 *   rank      after each stored factor r_e -= sigma u[row_e] v[col_e] and test_mse = sum r_e^2 / n_test (0 without test entries) goes to
 *             out_test_loss; a value strictly below the best so far resets the counter, anything else counts, and the loop ends when the
 *             counter reaches *patience -- with a fixed k_max too -- before the sigma < 100 eps stop (deflation.hpp:869-911)
 * *test_fraction = 0: no hold-out, out_test_loss untouched, *out_k_selected = *out_k_computed; without an obs_mask this is
 * rcppml_gpu_svd_pca_* with *algorithm 0, bit for bit.  obs_mask_p = NULL: no mask (the other obs_mask pointers are then not read); else a
 * pattern CSC with the dimensions of A and strictly increasing rows within a column.
 * Outputs: U (m x *k_max) and V (n x *k_max) column-major and d with the first *out_k_selected columns / values written; *out_k_computed
 * factors were computed, out_test_loss and out_iters_per_factor (each *k_max long) hold that many values; *out_n_test test entries;
 * *out_n_masked stored entries (dense: positions) the obs_mask zeroed; out_row_means (m) when *center.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), nothing written: a null pointer, *precision not RCPPML_F32 / RCPPML_F64, *k_max
 * outside [1, min(m, n)] or above 4094, *max_iter < 1, *patience < 1, *test_fraction outside [0, 1), negative *tol, a malformed matrix
 * or mask CSC, mask dimensions that differ from A's, more device memory than is free, no device. */
RCPPML_GPU_API void rcppml_gpu_svd_cv_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* test_fraction, int* cv_seed, int* patience,
        int* mask_zeros, const int* obs_mask_p, const int* obs_mask_i, int* obs_mask_rows, int* obs_mask_cols, int* obs_mask_nnz,
        double* U, double* d, double* V, int* out_k_selected, int* out_k_computed, double* out_test_loss, int* out_n_test,
        int* out_n_masked, int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);
RCPPML_GPU_API void rcppml_gpu_svd_cv_dense_ex(const double* A_data, int* m, int* n,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* test_fraction, int* cv_seed, int* patience,
        int* mask_zeros, const int* obs_mask_p, const int* obs_mask_i, int* obs_mask_rows, int* obs_mask_cols, int* obs_mask_nnz,
        double* U, double* d, double* V, int* out_k_selected, int* out_k_computed, double* out_test_loss, int* out_n_test,
        int* out_n_masked, int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);

/* L21, angular and graph-regularised deflation SVD (rcppml_amd/csrc/ops_svd.hip, kernels_svd_reg.hip.h).  BUILD-DEFINED: the reference has
 * no such symbols; its CPU deflation loop applies the three terms between the element constraints and the normalisation, on both sides, in
 * every iteration, with or without cross-validation (svd/deflation.hpp:191-292, :734-742, :779-787), and the four rcppml_gpu_svd_pca_*
 * entries still refuse them.  The parameters are rcppml_gpu_svd_cv_ex's, in order, with the new ones after ub_v; everything said there
 * (hold-out, *mask_zeros, obs_mask, patience, auto-rank, centering, the element constraints, the outputs) holds here and combines with
 * the new terms.  Per side and per iteration, on the freshly divided update x with nsq = |u_hat|^2 (v side) or |v|^2 (u side), times the
 * denominator correction under CV -- the number the element constraints take:
 *   L21      *L21 > 0 and |x|_2 > 1e-10 (cast to the working precision): L2_eff = L2 + *L21 / |x|_2, |x|_2 taken before any shrinkage;
 *            the L2 -> L1 -> nonneg -> upper-bound chain then runs with L2_eff (:200-213)
 *   angular  *angular > 0 and factor k > 0: x -= (*angular / nsq) F (F' x), F the k stored factors of that side, F' x taken from x
 *            after the element chain (:256-267)
 *   graph    graph_*_p != NULL and *graph_*_lambda > 0: x -= (*lambda / nsq) (L x), L the dim x dim CSC exactly as passed (L x, not L' x;
 *            L need not be symmetric), x the vector after the angular step (:283-292).  A gradient step, not a solve: it amplifies the
 *            high end of L's spectrum once *lambda * lambda_max(L) / nsq passes 1, as the reference does.
 * Normalisation, the break rules, momentum, the warm start, Gram-Schmidt, the Rayleigh quotient, the test loss and patience are the cv
 * entry's; none of the three terms touches the warm start or the Rayleigh quotient.  graph_*_p = NULL or *graph_*_lambda <= 0: no graph on
 * that side (the other five pointers of that side are then not read).  With *L21_*, *angular_* and both graphs off the call is
 * rcppml_gpu_svd_cv_ex, bit for bit and launch for launch.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), nothing written: everything rcppml_gpu_svd_cv_ex refuses; a negative or non-finite
 * *L21_*, *angular_* or *graph_*_lambda; *graph_u_dim != m or *graph_v_dim != n; a malformed graph CSC (the checks A gets); a non-finite
 * graph value; more device memory than is free, the graphs counted. */
RCPPML_GPU_API void rcppml_gpu_svd_reg_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u,
        double* angular_v, const int* graph_u_p, const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz,
        double* graph_u_lambda, const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim,
        int* graph_v_nnz, double* graph_v_lambda, double* test_fraction, int* cv_seed, int* patience, int* mask_zeros,
        const int* obs_mask_p, const int* obs_mask_i, int* obs_mask_rows, int* obs_mask_cols, int* obs_mask_nnz,
        double* U, double* d, double* V, int* out_k_selected, int* out_k_computed, double* out_test_loss, int* out_n_test,
        int* out_n_masked, int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);
RCPPML_GPU_API void rcppml_gpu_svd_reg_dense_ex(const double* A_data, int* m, int* n,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u,
        double* angular_v, const int* graph_u_p, const int* graph_u_i, const double* graph_u_x, int* graph_u_dim, int* graph_u_nnz,
        double* graph_u_lambda, const int* graph_v_p, const int* graph_v_i, const double* graph_v_x, int* graph_v_dim,
        int* graph_v_nnz, double* graph_v_lambda, double* test_fraction, int* cv_seed, int* patience, int* mask_zeros,
        const int* obs_mask_p, const int* obs_mask_i, int* obs_mask_rows, int* obs_mask_cols, int* obs_mask_nnz,
        double* U, double* d, double* V, int* out_k_selected, int* out_k_computed, double* out_test_loss, int* out_n_test,
        int* out_n_masked, int* out_iters_per_factor, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);

/* Constrained block SVD, Krylov-Seeded Projected Refinement (rcppml_amd/csrc/ops_svd.hip, kernels_svd_krylov.hip.h).  BUILD-DEFINED:
 * the reference runs this as algorithm 4 with element constraints (svd/krylov.hpp:262-796), which the four rcppml_gpu_svd_pca_*
 * entries still refuse.  Scope: L1, L2, nonneg and upper bound on either side, centering, FACTOR convergence.
 *   seed      V0 = NULL: Phase 1, the Lanczos of rcppml_gpu_svd_pca_* (algorithm 2, *max_iter 0, the caller's *tol, *center, *seed, no
 *             constraints), and k_actual is what it selected.  Else V0 is the n x *k_max column-major seed and k_actual = *k_max.  Only
 *             V of a seed is read: the first W-update overwrites W and d.
 *   pass      G = V'V, diagonal += 1e-12 + *L2_u; B = A V (centred: - mu (1'V)); W = B G^-1; per column with nsq = |V_c|^2 (the Gram's
 *             diagonal before the ridge): nsq <= 0 zeroes it (d_c = 0); else soft threshold *L1_u / (2 nsq), max(0, .) with *nonneg_u,
 *             min(*ub_u, .) with *ub_u > 0; d_c = |column| when above 100 eps, else 0; column /= d_c where d_c > 0.  L2 is not applied
 *             again in the projection.  Then the same for V with A'W - 1 (mu'W) and the _v values; d is overwritten.
 *             The k x k reduction, ridge, factorisation and inverse run in fp64 in both precisions (the reference's float path adds
 *             a ridge below fp32's epsilon).
 *   stop      from the second pass on dW = |W - W_prev|_F / (|W_prev|_F + eps) goes to out_dw, and dW < *tol ends the loop after that
 *             pass; at most *max_iter passes, or max(10, 2 ceil(log2 k_actual) + 3) when *max_iter <= 0.
 *   result    with nonneg, L1 or an upper bound on either side: the factors ordered by d descending (ties by index); with L2 only:
 *             QR of W diag(d) and of V and the SVD of R_w R_v', on the host in fp64 (signs of a column pair are not the reference's).
 * Outputs: U (m x *k_max) and V (n x *k_max) column-major and d with the first *out_k_selected (= k_actual) columns / values written;
 * *out_passes; out_dw (capacity: the pass limit) holds *out_passes - 1 values; out_row_means (m) when *center.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), nothing written: a null pointer (V0 aside), *precision not RCPPML_F32 /
 * RCPPML_F64, *k_max outside [1, min(m, n)] or above 128, a negative or non-finite *tol, penalty or bound, no element constraint at all
 * (that is Lanczos: rcppml_gpu_svd_pca_*), a non-finite V0, a malformed CSC, more device memory than is free, no device, a non-positive
 * Cholesky pivot (the message names the pass and the update). */
RCPPML_GPU_API void rcppml_gpu_svd_krylov_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, const double* V0, double* U, double* d, double* V,
        int* out_k_selected, int* out_passes, double* out_dw, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);
/* The same for a column-major dense matrix, read as a full CSC; with V0 = NULL its Lanczos seed is rcppml_gpu_svd_pca_dense_*'s. */
RCPPML_GPU_API void rcppml_gpu_svd_krylov_dense_ex(const double* A_data, int* m, int* n,
        int* precision, int* k_max, double* tol, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u,
        double* L2_v, int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, const double* V0, double* U, double* d, double* V,
        int* out_k_selected, int* out_passes, double* out_dw, double* out_frobenius_norm_sq, double* out_row_means,
        double* out_wall_time_ms, int* out_status);

/* Randomized block SVD (rcppml_amd/csrc/ops_svd.hip, kernels_svd_rand.hip.h).  BUILD-DEFINED: the reference's CPU method
 * randomized_svd (svd/randomized.hpp:59-241, Halko-Martinsson-Tropp), which the four rcppml_gpu_svd_pca_* entries run as Lanczos
 * under algorithm 3.  A fixed cost and no convergence test:
 *   sizes     p = min(max(10, k / 5), min(m, n) - k), l = k + max(p, 0) (refused above 128), q = 3 when *max_iter <= 0, else
 *             min(*max_iter, 10).
 *   sketch    Omega (n x l), Omega(i, j) = uniform<T>() - 0.5 from draw j n + i of the SplitMix64 stream of *seed (0: 42), filled on
 *             the device.
 *   steps     Y = A~ Omega; q times: Q = orth(Y), Z = orth(A~' Q), Y = A~ Z; then Q = orth(Y), Bt = A~' Q.  A~ is A, or with *center
 *             A minus its row means (never formed: A~ X = A X - mu (1'X), A~' X = A' X - 1 (mu'X)).  orth() is CholeskyQR2 in place of
 *             the reference's Householder QR (the thin factor is the same up to column signs, which cancel in U d V'): the l x l Gram
 *             and its factor are fp64 in both precisions, always two rounds.  A pivot that is not above l eps(T) times its column's
 *             Gram diagonal (or is NaN) zeroes that column of Q and the factorisation goes on: rank-deficient input is no error.
 *   result    the eigensystem of the l x l Gram Bt'Bt on the host in fp64: d = sqrt(lambda) descending, U = Q Vb, V = Bt Vb / d (a
 *             zero column where d = 0).  Singular values below sqrt(eps) d_1 are not resolved.  The answer is the method's
 *             approximation of the truncated SVD, not the truncated SVD.
 * Outputs: U (m x *k_max) and V (n x *k_max) column-major and d, all *out_k_selected = *k_max columns / values written;
 * out_iters_per_factor[0] = q; out_row_means (m) when *center.  Two runs are bitwise equal.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), nothing written: a null pointer (the graph and obs_mask pointers aside, where
 * null means none), *precision not RCPPML_F32 / RCPPML_F64, *k_max outside [1, min(m, n)], l above 128 (the message names l and the
 * limit), any of L1 / L2 / nonneg / upper bound / L21 / angular set, a graph pointer with its lambda above 0, *test_fraction > 0, a
 * non-null obs_mask_p (the reference's method supports none of them), a malformed CSC, a non-finite value, more device memory than is
 * free, no device. */
RCPPML_GPU_API void rcppml_gpu_svd_randomized_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* precision, int* k_max, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u, double* L2_v,
        int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        const int* graph_u_p, double* graph_u_lambda, const int* graph_v_p, double* graph_v_lambda, double* test_fraction,
        const int* obs_mask_p, double* U, double* d, double* V, int* out_k_selected, int* out_iters_per_factor,
        double* out_frobenius_norm_sq, double* out_row_means, double* out_wall_time_ms, int* out_status);
/* The same for a column-major dense matrix, read as a full CSC (svd/randomized.hpp is one template for both). */
RCPPML_GPU_API void rcppml_gpu_svd_randomized_dense_ex(const double* A_data, int* m, int* n,
        int* precision, int* k_max, int* max_iter, int* center, int* seed, double* L1_u, double* L1_v, double* L2_u, double* L2_v,
        int* nonneg_u, int* nonneg_v, double* ub_u, double* ub_v, double* L21_u, double* L21_v, double* angular_u, double* angular_v,
        const int* graph_u_p, double* graph_u_lambda, const int* graph_v_p, double* graph_v_lambda, double* test_fraction,
        const int* obs_mask_p, double* U, double* d, double* V, int* out_k_selected, int* out_iters_per_factor,
        double* out_frobenius_norm_sq, double* out_row_means, double* out_wall_time_ms, int* out_status);

/* SVD-seeded NMF start (rcppml_amd/csrc/ops_svd.hip, nmf_start_kernel in kernels_svd.hip.h).  BUILD-DEFINED: the reference's
 * initialize_lanczos / initialize_irlba (nmf/nmf_init.hpp:45-158), which its fits run for init_mode 1 / 2 (R: nmf(seed = "lanczos" |
 * "irlba")).  The plugin's NMF ABI (gpu/bridge_nmf.hpp) carries no init_mode: a caller runs this entry and hands W_T and H to a
 * fit entry as its start.
 *   svd       Golub-Kahan-Lanczos as rcppml_gpu_svd_pca_* run it under algorithm 2, in *precision, with the reference's fixed
 *             options: tol 1e-10, max_iter 0 (at most max(3k, k + 50) steps), no centring, the start vector of *seed (0: 42).
 *             *mode: 1 Lanczos, 2 IRLBA -- both run this engine, as algorithm 1 does on the svd entries.
 *   start     for c < *out_k_svd: W_T(c, i) = |u_c(i)| sqrt(sigma_c), H(c, j) = |v_c(j)| sqrt(sigma_c), the square root taken of
 *             sigma_c in the compute type, written on the device straight into the k x m / k x n column-major layout.
 *   fill      rows *out_k_svd .. k - 1 (Lanczos broke down early: a rank-deficient matrix) are uniform draws in the compute type
 *             from one sequential SplitMix64 stream seeded (uint32)*seed == 0 ? 54321 : (uint32)(*seed + 999) (0 after the wrap:
 *             12345, rng.hpp:73-74): first the (k - k_svd) x m block of W_T column by column, then the block of H
 *             (nmf_init.hpp:82-90).
 * Outputs: W_T (k x m) and H (k x n) column-major, every value written; d: the *out_k_svd singular values (d[c] for
 * c >= *out_k_svd is not written); *out_iters: the Lanczos steps run.  Two runs are bitwise equal.
 * Refused with *out_status = -1 (rcppml_gpu_last_error), nothing written: a null pointer, *precision not RCPPML_F32 / RCPPML_F64,
 * *k outside [1, min(m, n)], *mode not 1 or 2, more than 4095 Lanczos steps, a malformed CSC, a non-finite value, more device
 * memory than is free, no device. */
RCPPML_GPU_API void rcppml_gpu_nmf_svd_init_ex(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* precision, int* k, int* seed, int* mode, double* W_T, double* H, double* d, int* out_k_svd, int* out_iters,
        double* out_wall_time_ms, int* out_status);
/* The same for a column-major dense matrix, through the engine's dense products (no CSC copy is made). */
RCPPML_GPU_API void rcppml_gpu_nmf_svd_init_dense_ex(const double* A_data, int* m, int* n,
        int* precision, int* k, int* seed, int* mode, double* W_T, double* H, double* d, int* out_k_svd, int* out_iters,
        double* out_wall_time_ms, int* out_status);

/* BUILD-DEFINED, for tools/init_bench.py: device milliseconds of one nmf_start_kernel launch and of the one ritz_kernel launch it
 * replaces, on a *len x *ja basis of uniform draws with *kc of *k columns wanted: each the median of *reps launches after a warm-up,
 * timed between two events on the stream.  Refused (-1, nothing written): a null pointer, a bad *precision, *len < 1, *ja or *k
 * outside [1, 4095], *kc outside [1, *k], *reps outside [1, 1000], more device memory than is free, no device. */
RCPPML_GPU_API void rcppml_hip_nmf_start_time(int* precision, int* len, int* ja, int* kc, int* k, int* reps, double* out_start_ms,
        double* out_ritz_ms, int* out_status);

/* Embedding assessment (rcppml_amd/csrc/ops_assess.hip): the reference plugin's rcppml_gpu_assess (src/gpu_bridge_assess.cu:358-753)
 * with its 26 pointers, called by R's assess() (R/assess.R:708-769).  embedding: n x dim row-major doubles, cast to fp32.  Seeds are
 * (unsigned)*seed plus an offset (restart r: + r; silhouette: + 100; folds: + 200), each driving std::mt19937 + std::shuffle.
 *   do_clustering: *kmeans_nstart restarts of exactly *kmeans_maxiter assign / accumulate / divide steps from the points
 *     idx[c % n] of the restart's shuffle, n_centers = *n_classes; ARI and NMI of the best restart by ARI (strict >).  nstart < 1:
 *     both -1.  Deviation: the centroid sums are fp64 in a fixed order, rounded to fp32 and divided in fp32 (the reference adds fp32
 *     atomics, which has no fixed answer).
 *   do_silhouette: min(spc, class size) shuffled samples per class; mean silhouette over the points.
 *   do_classify: stratified *knn_folds-fold kNN vote (k = min(knn_k, n_train)); mean accuracy and macro F1 over all classes.
 *   do_batch && n_batch > 1: the min(batch_knn_k, n - 1) nearest non-self neighbours; mean normalised batch entropy and kNN
 *     batch silhouette.
 * Exact fp32 kNN: the k smallest candidates in (d, index) order, d >= 1e30 or NaN never chosen.  Outputs of metrics not asked for
 * are untouched.  Refused (*out_status = -1, nothing else written, reason in rcppml_gpu_last_error): n < 1, dim < 1; clustering
 * with kmeans_maxiter < 1 or n_classes < 1; classification with knn_k < 1 or knn_folds < 1; batch with batch_knn_k < 1; a label
 * outside [0, n_classes) when clustering, silhouette or classification is asked; a batch label outside [0, n_batch) when batch
 * mixing is asked; no device. */
RCPPML_GPU_API void rcppml_gpu_assess(const double* embedding, int* n, int* dim, const int* labels, int* n_classes,
        const int* batch_labels, int* n_batch, int* do_clustering, int* do_silhouette, int* do_classify, int* do_batch,
        int* kmeans_nstart, int* kmeans_maxiter, int* sil_samples_per_class, int* knn_k, int* knn_folds, int* batch_knn_k,
        int* seed, double* out_ari, double* out_nmi, double* out_silhouette, double* out_knn_accuracy, double* out_knn_f1,
        double* out_batch_sil, double* out_batch_entropy, int* out_status);
/* rcppml_gpu_assess plus the per-item results.  Each extra output may be NULL (not written); the others are written when their
 * metric runs: out_assignments (n, the best restart's), out_restart_ari / out_restart_nmi (nstart), out_sil_point (n, fp32),
 * out_fold_ids (n), out_fold_accuracy / out_fold_f1 (knn_folds, NaN for a fold without training or test points),
 * out_batch_entropy_point / out_batch_sil_point (n).  *point_capacity, *restart_capacity, *fold_capacity: the lengths of those
 * buffers; a buffer that is written and too short is refused like the inputs above. */
RCPPML_GPU_API void rcppml_gpu_assess_ex(const double* embedding, int* n, int* dim, const int* labels, int* n_classes,
        const int* batch_labels, int* n_batch, int* do_clustering, int* do_silhouette, int* do_classify, int* do_batch,
        int* kmeans_nstart, int* kmeans_maxiter, int* sil_samples_per_class, int* knn_k, int* knn_folds, int* batch_knn_k,
        int* seed, double* out_ari, double* out_nmi, double* out_silhouette, double* out_knn_accuracy, double* out_knn_f1,
        double* out_batch_sil, double* out_batch_entropy, int* out_assignments, double* out_restart_ari, double* out_restart_nmi,
        float* out_sil_point, int* out_fold_ids, double* out_fold_accuracy, double* out_fold_f1, double* out_batch_entropy_point,
        double* out_batch_sil_point, int* point_capacity, int* restart_capacity, int* fold_capacity, int* out_status);
/* Exact fp32 brute-force kNN.  query: n_query x dim row-major; train: n_train x dim, or NULL for the query matrix itself (required by
 * mask modes 1 and 2).  mask_mode 0: every train point; 1: not the query's own index; 2: not the points of the query's group
 * (group: n_query ints in [0, n_groups)).  group_k (mode 2, may be NULL): n_groups ints in [0, k], the k of a query of that group.
 * out_idx / out_dist: n_query x k (capacity *out_capacity), the k smallest candidates in (d, index) order; empty slots -1 / 1e30. */
RCPPML_GPU_API void rcppml_gpu_knn_float(const float* query, int* n_query, const float* train, int* n_train, int* dim, int* k,
        int* mask_mode, const int* group, const int* group_k, int* n_groups, int* out_idx, float* out_dist, int* out_capacity,
        int* out_status);
/* Host only, no device work: the random plan rcppml_gpu_assess draws.  Each output may be NULL (not drawn).  out_init_idx:
 * kmeans_nstart x n_classes initial centroid points (capacity *init_capacity); out_sil_samples: the silhouette samples, class by
 * class (capacity *sil_capacity), out_sil_counts: n_classes counts min(spc, class size); out_fold_ids: n fold ids (capacity
 * *fold_capacity).  Refused: n < 1, n_classes < 1, a label outside [0, n_classes), knn_folds < 1 with out_fold_ids, a short buffer. */
RCPPML_GPU_API void rcppml_gpu_assess_plan(const int* labels, int* n, int* n_classes, int* kmeans_nstart, int* sil_samples_per_class,
        int* knn_folds, int* seed, int* out_init_idx, int* init_capacity, int* out_sil_samples, int* out_sil_counts,
        int* sil_capacity, int* out_fold_ids, int* fold_capacity, int* out_status);

/* Distribution diagnostics (rcppml_amd/csrc/ops_distribution.hip): the device side of the reference's score_test_distribution,
 * diagnose_zero_inflation and diagnose_dispersion (R/auto_distribution.R:194-452), fp64, with mu = (W diag(d)) H formed a tile at a
 * time and never stored.  Build-defined: R does not call these entries.  The matrix comes as a CSC (col_ptr, row_idx, values, *nnz)
 * or as a column-major m x n dense array: exactly one of col_ptr and dense is non-NULL.  The model: W_T (k x m), d (k), H (k x n).
 * Refused (*out_status = -1, reason in rcppml_gpu_last_error, no output written): m, n or k below 1; both matrix forms or neither;
 * a malformed CSC (row indices strictly increasing within each column); a non-finite value in the matrix or the model; arguments
 * outside their range; a call that does not fit in free device memory (the message gives the byte count); no device.
 *
 * Score test over the observed entries (sparse: the stored values != 0; dense: all m*n), mu' = max(mu, *min_mu), r = x - mu':
 * out_T[q] = mean(r^2 / mu'^powers[q] - 1) (1 <= *n_powers <= 8), *out_T_nb = mean((r^2 - mu') / mu'^2), *out_all_integer = every
 * observed x integral, *out_count = the number of observed entries.  mu'^p is mu' * mu' for p = 2, 1 for p = 0, pow otherwise. */
RCPPML_GPU_API void rcppml_gpu_score_test_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* k, const double* W_T, const double* d, const double* H, const double* powers,
        int* n_powers, double* min_mu, double* out_T, double* out_T_nb, int* out_all_integer, int64_t* out_count, int* out_status);
/* Zero inflation: out_expected_row (m) / out_expected_col (n) = row / column sums of exp(-max(mu, 1e-8)) over all m*n entries;
 * out_observed_row / out_observed_col = zeros per row / column (sparse: n - stored entries of the row, m - stored entries of the
 * column, explicit zeros counting as stored; dense: entries == 0). */
RCPPML_GPU_API void rcppml_gpu_zero_inflation_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* k, const double* W_T, const double* d, const double* H, double* out_expected_row,
        double* out_expected_col, double* out_observed_row, double* out_observed_col, int* out_status);
/* Dispersion: phi = (x - mu')^2 / mu'^*power over all m*n entries (x = 0 where a CSC stores nothing), mu' = max(mu, *min_mu);
 * trimmed means (R's mean(x, trim): the mean of the order statistics floor(N trim) + 1 .. N - floor(N trim), 0 <= *trim < 0.5)
 * per row (out_row_phi, m), per column (out_col_phi, n) and over all entries (*out_global_phi).  Needs 8 m n bytes of device memory
 * for phi beyond the inputs. */
RCPPML_GPU_API void rcppml_gpu_dispersion_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* k, const double* W_T, const double* d, const double* H, double* power,
        double* min_mu, double* trim, double* out_row_phi, double* out_col_phi, double* out_global_phi, int* out_status);

/* Consensus clustering (rcppml_amd/csrc/ops_consensus.hip): what the reference's consensus_nmf does after its fits
 * (R/consensus.R:102-137).  Build-defined: R has no hook for these entries (its consensus stage runs in R and in c_knn_jaccard,
 * src/RcppFunctions_utils.cpp:560-618).
 *
 * rcppml_gpu_consensus_double, on the device, replaces R/consensus.R:102-129 and c_knn_jaccard.  W_stack: *reps replicates, each
 * k x m column-major like the ABI's W (sample i = k contiguous values).  *method 0 (hard): label = first maximum of a sample's k
 * values (which.max), out_consensus[i, j] = (replicates with equal labels) / reps; out_labels (reps x m, 0-based, may be NULL) is
 * written for this method only.  *method 1 (knn_jaccard), per replicate: samples scaled to unit 2-norm, sim = Wn Wn^T in fp64,
 * actual_k = min(*knn, m - 1), the neighbour set of i = the actual_k largest sim[i, j], j != i,
 * J[i, j] = |Si & Sj| / (2 actual_k - |Si & Sj|) (0 when the denominator is 0, 1 on the diagonal), J added in replicate order and
 * divided by reps.  Two rules of this build where the reference is undefined: equal similarities go to the lower index
 * (std::partial_sort leaves ties open), and a sample with zero norm has similarity 0 to every sample (R: NaN).  out_consensus: m x m
 * (symmetric).  Device memory: 8 m^2 + the W stack + 4 reps m (hard) or 8 m ceil(m / 64) + a sim strip of at most 64 MiB
 * (knn_jaccard).  Refused (*out_status = -1, reason in rcppml_gpu_last_error, no output written): a null pointer, m < 2, k < 1,
 * reps < 1, method outside {0, 1}, knn < 1, a non-finite value in W_stack (negative values are accepted, as R accepts them), no HIP
 * device, not enough free device memory (the message gives the byte count). */
RCPPML_GPU_API void rcppml_gpu_consensus_double(const double* W_stack, int* m, int* k, int* reps, int* method, int* knn,
        double* out_consensus, int* out_labels, int* out_status);
/* Host only, no device work: hclust(as.dist(dist), "average"), cutree(k = *k_cut) and cor(as.dist(dist), cophenetic(hc))
 * (replaces R/consensus.R:133-137).  dist: m x m column-major, only the entries below the diagonal are read.  Each step merges the
 * pair with the smallest dissimilarity; among equal minima the pair with the smallest lower index, then the smallest upper index
 * (this build's rule; believed to be R's hclust, not verified against R).  The merged cluster keeps the lower slot and is updated by
 * Lance-Williams, (na da + nb db) / (na + nb).  out_merge: (m - 1) x 2 column-major in R's convention (negative: sample, 1-based;
 * positive: step, 1-based; samples before clusters, the lower sample or earlier step first); out_height (m - 1): the merge
 * dissimilarities; out_clusters (m): the last k_cut - 1 merges undone, clusters numbered 1..k_cut by first appearance;
 * *out_cophenetic: Pearson correlation over the m (m - 1) / 2 pairs (two-pass, clamped to [-1, 1]), NaN when all dissimilarities or
 * all merge heights are equal.  Refused: a null pointer, m < 2, k_cut outside [1, m], a non-finite dissimilarity. */
RCPPML_GPU_API void rcppml_gpu_hclust_average_double(const double* dist, int* m, int* k_cut, int* out_merge, double* out_height,
        int* out_clusters, double* out_cophenetic, int* out_status);

/* Label-guided refinement (rcppml_amd/csrc/ops_refine.hip): the reference's compute_target() (R/compute_target.R:65-121) and
 * refine() without a batch (R/refine.R:109-187), fp64.  Build-defined: R has no hook for these entries.  H: k x n column-major (k
 * leading); labels: n ints in 0 .. *n_classes - 1, a negative value is R's NA (the column is unguided).  The per-class sums, ||H||_F^2
 * and the correction run on the device; the k x C stage (centroids, OAS shrinkage, cyclic-Jacobi eigendecomposition, ZCA, shifts)
 * on the host.  Results are bitwise-repeatable: no atomics, every summation order is fixed by (k, n, the labels).
 * Refused (*out_status = -1, reason in rcppml_gpu_last_error, no output written): a null pointer; k, n or m below 1; n_classes < 0;
 * a label >= n_classes; lambda outside [0, 1]; cycles < 0; both matrix forms or neither; a malformed CSC (row indices strictly
 * increasing within a column); a non-finite value in H, W, d or the matrix; k > 64 where a refit runs; not enough free device
 * memory (the message gives the byte count); no HIP device.
 *
 * rcppml_gpu_compute_target_double: out_target (k x n) = shift[, label_j] (0 for NA).  centroid_c = the class mean (0 for an empty
 * class); grand_mean = the mean of the non-empty classes' centroids.  *whiten and n_classes > 1: X = (centroids - grand_mean)
 * sqrt(max(count, 1)), S = X X^T / sum(count), rho = ((1 - 2/k) tr(S^2) + tr(S)^2) / ((sum(count) + 1 - 2/k) (tr(S^2) - tr(S)^2 / k))
 * clamped to [0, 1] (1 when |denominator| < 1e-12), S_shrunk = (1 - rho) S + rho tr(S) / k I, W_zca = V diag(1 / sqrt(max(eig,
 * 1e-10))) V^T applied to the centroids and to grand_mean.  shift = centroids - grand_mean.  out_shift (k x n_classes) and
 * out_counts (n_classes) may be NULL. */
RCPPML_GPU_API void rcppml_gpu_compute_target_double(const double* H, const int* labels, int* k, int* n, int* n_classes, int* whiten,
        double* out_target, double* out_shift, int* out_counts, int* out_status);
/* Stage 1 of refine() (R/refine.R:109-122): out_H_corr = H + *lambda * s * T with T the target above and s = ||H||_F / ||T||_F
 * (applied only when ||T||_F > 1e-10), clipped at 0 when *nonneg.  out_target (k x n, the unscaled T) may be NULL. */
RCPPML_GPU_API void rcppml_gpu_refine_correct_double(const double* H, const int* labels, int* k, int* n, int* n_classes, int* whiten,
        double* lambda, int* nonneg, double* out_H_corr, double* out_target, int* out_status);
/* The W refit of a refine() cycle alone (R/refine.R:137-145): out_W (k x m) = solve(G + 1e-8 I, B) with dH = diag(d) H_corr,
 * G = dH dH^T, B = A dH^T, clipped at 0 when *nonneg (an unconstrained solve and a clip, not NNLS).  The matrix: a host CSC
 * (col_ptr, row_idx, values, *nnz) or a column-major m x n dense array, exactly one of the two. */
RCPPML_GPU_API void rcppml_gpu_refine_wfit_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* k, const double* d, const double* H_corr, int* nonneg, double* out_W,
        int* out_status);
/* refine(): stage 1, then *cycles cycles of (R/refine.R:135-187): the W refit above; H = solve(W^T W + 1e-8 I, W^T A), clipped
 * when *nonneg; d = the L2 row norms of H floored at 1e-10, H divided by d, W multiplied by d; stage 1 again on the new H.  W_T
 * (k x m), d (k), H (k x n) are read only; out_W, out_d, out_H: the model after the cycles (the inputs when *cycles = 0: the matrix may
 * then be absent, both pointers NULL); out_H_corr: the corrected H.  The matrix and the factors stay on the device between cycles. */
RCPPML_GPU_API void rcppml_gpu_refine_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* k, const double* W_T, const double* d, const double* H, const int* labels,
        int* n_classes, double* lambda, int* cycles, int* nonneg, int* whiten, double* out_W, double* out_d, double* out_H,
        double* out_H_corr, int* out_status);

/* Zero-inflated GP / NB NMF (rcppml_amd/csrc/ops_zi.hip, kernels_zi.hip.h).  Build-defined: the reference's bridge has no slot for zi and
 * its device path ignores it, so the specification is the reference's CPU fit, inst/include/FactorNet/nmf/fit_cpu.hpp:
 *   :350-400    pi_row[i] = min(0.5 (1 - nnz_row_i / n), 0.3), pi_col[j] = min(0.5 (1 - nnz_col_j / m), 0.3), counts of STORED entries
 *               (an entry is a zero iff the CSC does not store it; an explicit stored 0 is not a zero);
 *   :403-421    A_imputed = A as a dense matrix;
 *   :589-596, :833-840  from ALS iteration 1 on both half-updates are the dense IRLS (every entry weighted, each batch from zero) on
 *               A_imputed and its transpose; iteration 0 is the plain sparse IRLS fit's;
 *   :1285-1479  after the W update and the dispersion update (on the original A) of EVERY iteration: zi_em_iters rounds of the E-step
 *               over the unstored (i, j) -- s = max((W_T o d)_i . h_j, 1e-10); NB p0 = (r_i / (r_i + s))^r_i, r_i = max(size_i, 1e-10);
 *               GP p0 = exp(-s / (1 + theta_i)); z = pi / (pi + (1 - pi) p0 + 1e-300), summed per row (ROW) or column (COL) -- and the
 *               M-step pi = clamp(zsum / n, 0.001, 0.999) (ROW; COL: / m) where the row / column has an unstored entry, each round
 *               followed by theta_i = max(theta_i, gp_theta_min) (GP, gp_theta_min > 0);
 *   :1490-1550  one imputation A_imputed(i, j) = z s at the unstored entries with the UPDATED pi, stored entries keep A's value;
 *   :1684-1767  then the loss, on the original A's stored entries;  :1837-1840 pi_row / pi_col are returned.
 * Scope: fp64, a host CSC (row indices strictly increasing within a column), the CD solver, k <= 128, L1 / L2 / nonneg / upper bounds
 * as the IRLS path takes them, dispersion none / global / per row.  fp32, dense input, masks, cross-validation and several devices are
 * not offered under ZI.  Refused (*out_status = -1, reason in rcppml_gpu_last_error, NO output buffer written): zi_mode 3 (TWOWAY,
 * with the text of core/config.hpp:437-440) or outside {1 ROW, 2 COL}; a loss other than GP (4) / NB (5); dispersion mode 3 (per_col:
 * the reference indexes the dispersion vector by row in the E-step); k > 128; zi_em_iters < 1; a malformed CSC; a null pointer; a
 * call whose device arrays -- two m x n fp64 arrays, two m n int32 index arrays, the bitmask (m n / 8 bytes), the tile partials --
 * exceed the free device memory (checked by arithmetic before anything is allocated; the message gives the byte count); m n >= 2^31;
 * no HIP device.
 * Results are bitwise-repeatable and independent of the launch grid: no floating-point atomics, per-tile partials in a fixed order
 * added in tile order.
 *
 * rcppml_gpu_nmf_zi_double: W (k x m), H (k x n), d (k) in/out as in rcppml_gpu_nmf_ex; loss_history (>= *max_iter doubles) may be NULL;
 * out_theta holds m doubles (*out_theta_len returns m); out_pi holds max(m, n) doubles, *out_pi_len returns m (ROW) or n (COL).
 * *sort_model orders the factors by descending d; pi is per row / column and is not permuted. */
RCPPML_GPU_API void rcppml_gpu_nmf_zi_double(const int* col_ptr, const int* row_idx, const double* values, int* m, int* n, int* nnz,
        int* k, double* W, double* H, double* d, int* max_iter, double* tol, double* L1_H, double* L1_W, double* L2_H, double* L2_W,
        double* ub_H, double* ub_W, int* cd_maxit, double* cd_tol, int* verbose, int* patience, int* nonneg_W, int* nonneg_H,
        int* loss_type, int* irls_max_iter, double* irls_tol, int* norm_type, int* dispersion_mode, double* gp_theta_init,
        double* gp_theta_max, double* gp_theta_min, double* nb_size_init, double* nb_size_max, double* nb_size_min, int* sort_model,
        int* zi_mode, int* zi_em_iters, double* loss_history, double* out_theta, int* out_theta_len, double* out_pi, int* out_pi_len,
        int* out_iter, int* out_converged, double* out_loss, double* out_tol, int* out_status);
/* The stage alone (fit_cpu.hpp:1285-1552): *zi_em_iters rounds of E-step, M-step and theta floor, then one imputation.  W_T (k x m), d
 * (k), H (k x n) are read; disp (m: NB sizes or GP theta) is in/out (floored for GP when *theta_min > 0); pi (m for ROW, n for COL,
 * values in [0, 1]) is in/out; out_imputed (m x n column-major, may be NULL) receives A_imputed -- its stored entries are A's values
 * bit for bit.  Here m n may exceed 2^31 (64-bit indexing; no index arrays are built).  Env RCPPML_GPU_ZI_GRID = the number of
 * workgroups the tile kernels are launched with (a test hook: the result does not depend on it). */
RCPPML_GPU_API void rcppml_gpu_zi_em_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz, int* m, int* n,
        int* k, const double* W_T, const double* d, const double* H, double* disp, int* loss_type, int* zi_mode, int* zi_em_iters,
        double* theta_min, double* pi, double* out_imputed, int* out_status);

/* Classifier evaluation (rcppml_amd/csrc/ops_classify.hip): the device side of the reference's classify_embedding and
 * classify_logistic (R/classifier_metrics.R:49-138, 219-291) and of their metrics (.build_eval_result, .compute_auc, :387-492).
 * Build-defined: R does not call these entries.  Embeddings are row-major doubles (n x dim), labels int codes in [0, *n_classes).
 * Refused (*out_status = -1, reason in rcppml_gpu_last_error, NO output buffer written): a null pointer (out_launches and row_blocks
 * may be NULL), n_train < 1, n_test < 1, dim outside [1, 128], n_classes outside [2, 256], a label outside [0, n_classes), a
 * non-finite value, k outside [1, n_train], distance other than 0 / 1, maxit < 1, no device, or a call that does not fit in the free
 * device memory (the message carries the byte count).
 *
 * The metric outputs, shared by the three entries: out_predictions (n_test; the row argmax of the probabilities, first maximum on
 * ties), out_confusion (n_classes x n_classes row-major int counts, rows true, columns predicted), out_precision / out_recall /
 * out_f1 (n_classes; 0 when the denominator is 0), out_support (n_classes, the row sums), out_auc (n_classes; one-vs-rest, pairs
 * (positive i, negative j) with s_i > s_j, or s_i = s_j and i < j, counted in 64-bit integers and divided by n_pos n_neg; 0.5 when a
 * side is empty).
 *
 * rcppml_gpu_classify_metrics_ex: prob is n_test x n_classes row-major. */
RCPPML_GPU_API void rcppml_gpu_classify_metrics_ex(const double* prob, const int* test_labels, int* n_test, int* n_classes,
        int* out_predictions, int* out_confusion, double* out_precision, double* out_recall, double* out_f1, int* out_support,
        double* out_auc, int* out_status);
/* k nearest training rows of every test row (exact top-k by (fp32 squared distance, train index)); *distance 0 euclidean, 1 cosine
 * (rows scaled to unit norm, a zero norm taken as 1).  out_votes: n_test x n_classes, neighbour label counts / k.  *out_launches
 * (may be NULL): kernel launches of the call. */
RCPPML_GPU_API void rcppml_gpu_classify_knn_ex(const double* train, const double* test, const int* train_labels,
        const int* test_labels, int* n_train, int* n_test, int* dim, int* n_classes, int* k, int* distance, double* out_votes,
        int* out_predictions, int* out_confusion, double* out_precision, double* out_recall, double* out_f1, int* out_support,
        double* out_auc, int* out_launches, int* out_status);
/* n_classes one-vs-rest binomial(logit) GLMs on [1 | train] by IRLS with R's glm.fit arithmetic (*maxit 25 and *epsilon 1e-8 are
 * glm.control's), fp64, normal equations + Cholesky; a column whose pivot is <= 1e-11 x the largest diagonal entry is aliased
 * (coefficient 0).  out_coef / out_aliased: n_classes x (dim + 1), intercept first; out_iters / out_converged / out_deviance:
 * n_classes; out_prob: n_test x n_classes, rows divided by their sum (a zero sum taken as 1).  *row_blocks (may be NULL; 0: one
 * per 128-row chunk): the workgroups of the per-iteration pass, a test switch -- the results do not depend on it. */
RCPPML_GPU_API void rcppml_gpu_classify_logistic_ex(const double* train, const double* test, const int* train_labels,
        const int* test_labels, int* n_train, int* n_test, int* dim, int* n_classes, int* maxit, double* epsilon, int* row_blocks,
        double* out_coef, int* out_aliased, int* out_iters, int* out_converged, double* out_deviance, double* out_prob,
        int* out_predictions, int* out_confusion, double* out_precision, double* out_recall, double* out_f1, int* out_support,
        double* out_auc, int* out_launches, int* out_status);

/* Last error text of the calling thread ("" if none). */
RCPPML_GPU_API const char* rcppml_gpu_last_error(void);

/* --------------------------------------------------------------------------
 * (2) Device-level ops.  dtype: 0 = fp32, 1 = fp64.  All pointers are DEVICE pointers unless
 * named host_*.  Every op is enqueued on the context's stream and returns 0 on success
 * (non-zero: see rcppml_gpu_last_error).  No op synchronises the stream.
 * ------------------------------------------------------------------------*/
typedef struct rcppml_hip_ctx rcppml_hip_ctx;

enum { RCPPML_F32 = 0, RCPPML_F64 = 1 };
/* CD kernel variants (rcppml_hip_solve_cd `variant`) */
enum { RCPPML_CD_AUTO = 0 /* = GROUP unless RCPPML_GPU_CD_VARIANT says otherwise */,
       RCPPML_CD_LANE = 1 /* one lane per column, residual+iterate in registers, G through the scalar cache (SGPRs) */,
       RCPPML_CD_WAVE = 2 /* one wavefront per column, active-coordinate ballot skipping, G in LDS */,
       RCPPML_CD_GROUP = 5 /* 1, 2 or 4 adjacent lanes per column (DPP broadcasts), G from LDS */,
       RCPPML_CD_MFMA16 = 7 /* k <= 64, fp32 or fp64: 16 columns per wave, four coordinates per v_mfma_*_16x16x4 (the fp64 default) */,
       RCPPML_CD_MFMA = 6 /* fp32, k <= 128: residual tiles in MFMA accumulators, two coordinates per v_mfma_f32_32x32x2_f32 */,
       RCPPML_CD_LMF = 8 /* fp32, k <= 64, non-negativity only: lane = column, rank-1 updates as v_mfma_f32_4x4x1_16B blocks, persistent
                            waves with column refill (the fp32 default for NMF half-updates) */ };

/* stream: a hipStream_t (NULL = the device's null stream).  The context owns scratch memory only. */
RCPPML_GPU_API int rcppml_hip_ctx_create(rcppml_hip_ctx** out, int device, void* stream);
RCPPML_GPU_API void rcppml_hip_ctx_destroy(rcppml_hip_ctx* ctx);
RCPPML_GPU_API int rcppml_hip_ctx_sync(rcppml_hip_ctx* ctx);
/* Work counters since creation / the last reset (synchronises the stream): out4[0] = column-sweeps of the
 * coordinate-descent kernels (sum over solved columns of the sweeps cd_nnls_col_fixed ran, nnls_batch.hpp:127-131, i.e. the
 * sum of sweeps_out: at tol = 0 the static-sweep kernel counts maxit for a column it left at its fixed point, so there these
 * are sweeps reported, not executed; x 2 k_pad^2 = the flops of the residual updates), out4[1] = columns solved, out4[2] = slot-sweeps the persistent LMF
 * kernel executed (column slots x sweeps of their wave: idle slots and warm-start correction sweeps included, so
 * 1 - out4[0] / out4[2] is its idle fraction), out4[3] = coordinate steps of that kernel in which NO column of the wave
 * moved (only with RCPPML_OPT_CD_COUNT_NOOP; a step is one coordinate of one wave-sweep).  out4[0] and out4[1] are counted by
 * every kernel rcppml_hip_solve_cd dispatches to (LANE, WAVE and the general-rank kernel included), out4[2..3] by LMF. */
RCPPML_GPU_API int rcppml_hip_ctx_stats(rcppml_hip_ctx* ctx, int reset, unsigned long long* out4);
/* IRLS work counters (only while RCPPML_OPT_CD_COUNT_NOOP is set; two atomics per column): out2[0] = IRLS passes summed over
 * the columns rcppml_hip_solve_irls solved (nnls_batch_irls.hpp:480-560: each pass rebuilds the weighted Gram and solves),
 * out2[1] = the same weighted by the column's nonzeros = rank-1 updates f f^T of the weighted Grams (x 2 k_pad^2 = flops). */
RCPPML_GPU_API int rcppml_hip_ctx_irls_stats(rcppml_hip_ctx* ctx, int reset, unsigned long long* out2);
/* out1[0] = CD sweeps executed inside the IRLS half-updates (per column and pass, until the column's own fixed point); counted with the above */
RCPPML_GPU_API int rcppml_hip_ctx_irls_sweep_stats(rcppml_hip_ctx* ctx, int reset, unsigned long long* out1);
/* Per-(column, coordinate) step counters of the lane = column CD kernel (only while RCPPML_OPT_CD_COUNT_NOOP is set): out2[0] =
 * coordinate steps whose update is exactly 0 -- the steps the reference skips with `continue` (primitives/cpu/nnls_batch.hpp:
 * 102,106,109) and a dense sweep still executes --, out2[1] = all coordinate steps of live columns (warm-start correction
 * sweeps and padded coordinates excluded).  bench.py: roofline.useful_frac = frac x (1 - out2[0] / out2[1]). */
RCPPML_GPU_API int rcppml_hip_ctx_cd_step_stats(rcppml_hip_ctx* ctx, int reset, unsigned long long* out2);
/* Tuning / diagnostic switches of a context (0 = default behaviour for all of them). */
enum { RCPPML_OPT_CD_COUNT_NOOP = 1 /* LMF kernel counts all-zero coordinate steps into stats[3], IRLS kernels count passes (slower) */,
       RCPPML_OPT_CD_LMF_LANE_GROUPS = 2 /* 1, 2 or 4 lane groups per column instead of the size heuristic */,
       RCPPML_OPT_CD_LMF_WAVES_PER_SIMD = 3 /* resident persistent waves per SIMD instead of the heuristic */,
       RCPPML_OPT_CD_NO_LMF = 4 /* RCPPML_CD_AUTO falls back to the 32- / 16-column MFMA kernels */,
       RCPPML_OPT_IRLS_COLUMNS_PER_WAVE = 5, /* fp32 k <= 32 IRLS half-update: 0 = by the number of columns, 1 or 4 columns per wavefront */
       RCPPML_OPT_SMALL_GIVE_UP = 6 /* test switch: the one-kernel fit's first barrier gives up at once (its abort flag is preset), as if
                                       its workgroups had not all arrived on one XCD -- exercises the caller's restart on the multi-launch ops */,
       RCPPML_OPT_CD_PLACED = 7 /* launch form of the fp32 k <= 64 MFMA solves: 0 = explicitly placed (one workgroup per CU, static tile
                                   map) when there are 2 to 5 32-column tiles, or between 1 and 2 16-column tiles, per SIMD; 1 = explicitly
                                   placed whenever those kernels run; 2 = never (one workgroup per four tiles); 3 / 4 = as 0 for the 32- /
                                   16-column tiles only (A/B runs).  Same results bit for bit */,
       RCPPML_OPT_CD_ASSUME_CUS = 8 /* test switch: the explicitly placed launch assumes this many CUs (> 0) instead of the device's */,
       RCPPML_OPT_CD_PRIO = 9 /* wave priorities (s_setprio) in the fp32 k <= 64 MFMA solves with the plain non-negative step: value = mode of
                                 the 32-column tiles (the H side of a wide fit) + 8 x mode of the 16-column tiles (the W side).  Modes: 0 none;
                                 1 / 2 static by round of the explicitly placed launch, younger / older rounds boosted (the tile-per-wave
                                 launch ignores them); 3 / 4 dynamic, priority 1 during the scalar step / around the MFMAs of every
                                 coordinate pair or quad.  Any other value is refused.  A context starts at RCPPML_CD_PRIO_DEFAULT; unlike
                                 the other switches, 0 here means "no priorities", not "default".  Same results bit for bit */ };
#define RCPPML_CD_PRIO_DEFAULT 3 /* H side: priority 1 during the scalar step (mode 3); W side: none.  profiles/cd_prio_ab.txt */
RCPPML_GPU_API int rcppml_hip_ctx_set_option(rcppml_hip_ctx* ctx, int option, int value);

/* One-time setup of a fit, on the device.
 * rcppml_hip_transpose_csc: CSC of A^T from the CSC of A (rows x cols; all pointers device memory; t_col_ptr rows+1 ints,
 *   t_row_idx / t_values nnz entries; values / t_values may be NULL for a pattern-only matrix such as a mask).  Replaces the
 *   reference's host-side `At = A.transpose()` (nmf/fit_cpu.hpp:251-253): a stable sort by row index, so the column
 *   indices inside each row of A come out ascending, as Eigen produces them.  Synchronises the stream.
 * rcppml_hip_cast: elementwise precision cast between device buffers (the plugin boundary hands over doubles,
 *   gpu/bridge_nmf.hpp:310-342; the fp32 entry computes in fp32). */
RCPPML_GPU_API int rcppml_hip_transpose_csc(rcppml_hip_ctx* ctx, int dtype, int rows, int cols, const int* col_ptr,
                                            const int* row_idx, const void* values, int* t_col_ptr, int* t_row_idx,
                                            void* t_values);
/* The same transpose in two asynchronous steps (no stream synchronisation when the context serves temporaries from a per-fit
 * arena): _sort needs the index arrays only -- it makes the row pointers of A^T and the nonzero positions sorted by row
 * (sorted_pos: nnz ints; a stable counting sort over column chunks, own kernels) -- so the plugin runs it while the VALUES are
 * still crossing PCIe; _gather then fills t_row_idx / t_values (either
 * may be NULL: indices before the values have arrived, values after). */
RCPPML_GPU_API int rcppml_hip_transpose_csc_sort(rcppml_hip_ctx* ctx, int rows, int cols, int64_t nnz, const int* col_ptr,
                                                 const int* row_idx, int* t_col_ptr, int* sorted_pos);
RCPPML_GPU_API int rcppml_hip_transpose_csc_gather(rcppml_hip_ctx* ctx, int dtype, int cols, int64_t nnz, const int* col_ptr,
                                                   const int* sorted_pos, const void* values, int* t_row_idx, void* t_values);
RCPPML_GPU_API int rcppml_hip_cast(rcppml_hip_ctx* ctx, int dtype_src, const void* src, int dtype_dst, void* dst, int64_t n);

/* G = F F^T (+ eps on the diagonal, then + l2) -- reference primitives/cpu/gram.hpp:37-67 and
 * nmf/fit_cpu.hpp:506,738.  F: k x r.  MFMA kernel (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64),
 * split over r with a deterministic two-pass reduction. */
RCPPML_GPU_API int rcppml_hip_gram(rcppml_hip_ctx* ctx, int dtype, const void* F, int k, int64_t r,
                                   double eps, double l2, void* G);

/* B(:,j) = sum_{i in nz(j)} A(i,j) F(:,i) -- reference primitives/cpu/rhs.hpp:52-70 and the RHS
 * step of primitives/cpu/fused_nnls.hpp:109-114.  One wavefront per output column. */
RCPPML_GPU_API int rcppml_hip_rhs(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr,
                                  const int* row_idx, const void* values, int64_t ncols,
                                  const void* F, int k, void* B);

/* Planned form of the same product for large inputs (build-defined; the reference has one CPU loop, rhs.hpp:52-70).
 * A plan is a device copy of ONE CSC matrix for one rank k and precision, laid out for a kernel that stages the rows of F through
 * LDS and keeps the output columns in registers.  Two plan kinds (rcppml_hip_rhs_plan_kind says which the planner took):
 *   window plan (kind 1, kernels_rhs_win.hip.h -- the default): a ring of four 32 KiB row tiles, nonzeros scheduled over a sliding
 *     window of three tiles at a fractional slot rate; what the window cannot place (the "overflow", a few per cent) is added by
 *     the finishing pass that also sums the row partitions; no tail launch.  Declined (-> slab plan) for slot rates above 6 per
 *     phase, rows not sorted inside a column, hypersparse inputs, or more than 25 % overflow.
 *   slab plan (kind 0, kernels_rhs_tiled.hip.h -- the r2/r3 form, the fallback): 64 KiB tiles, S slots per (column, tile), the
 *     rest spilled to a gather kernel (refused above 35 % spill); columns that would only part-fill a last round of workgroups go
 *     to the gather kernel.
 *   plan_create: nrows = rows of the sparse matrix (= number of k-vectors in F).  partitions: 0 = automatic.
 *     slots: 0 = window plan, then slab plan, then no plan; 1 = slab plan with S chosen from the data; 2..8 = slab plan with S
 *     slots; >= 100 = window plan at (slots - 100) / 4 slots per column and phase (e.g. 107 = 1.75).
 *     *out_plan stays NULL (return 0) when no plan kind is eligible (k * sizeof(T) not 256 or 512 bytes -- or 1024 in fp64 --,
 *     unsorted rows, too irregular): call rcppml_hip_rhs then.
 *   rhs_planned: B = F * A(:, j) for all columns, same numbers as rcppml_hip_rhs up to summation order; deterministic.
 *     The plan keeps the col_ptr / row_idx / values POINTERS: the CSC must outlive the plan.
 *   plan_info (11 doubles): {P, waves per workgroup, rounds per wave, slots (slab: S; window: clo + nhi / 4 = the slot rate),
 *     workgroups per partition, tiles, slot count, spilled / overflow nonzeros, slot fill fraction, slot stream bytes, columns
 *     handled by the tiled kernel}.
 *   plan_set_values works only on plans made by plan_create_indices (it needs their per-nonzero destination table). */
typedef struct rcppml_rhs_plan rcppml_rhs_plan;
RCPPML_GPU_API int rcppml_hip_rhs_plan_create(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx,
                                              const void* values, int64_t ncols, int64_t nrows, int k, int partitions,
                                              int slots, rcppml_rhs_plan** out_plan);
/* The same plan in two steps: _create_indices does everything that needs only the index arrays (the schedule, the offsets, the
 * overflow lists, and for every nonzero where its value will go), _set_values scatters the values with one coalesced pass and
 * may be called again when the values of the same pattern change.  The plugin builds both plans while the values are still
 * crossing PCIe.  *out_plan = NULL when the window planner declines the input (use rcppml_hip_rhs_plan_create then). */
/* 1 = window plan, 0 = slab plan (see above), -1 = NULL. */
RCPPML_GPU_API int rcppml_hip_rhs_plan_kind(const rcppml_rhs_plan* plan);
RCPPML_GPU_API int rcppml_hip_rhs_plan_create_indices(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx, int64_t ncols,
                                                      int64_t nrows, int k, int partitions, int slots, rcppml_rhs_plan** out_plan);
RCPPML_GPU_API int rcppml_hip_rhs_plan_set_values(rcppml_hip_ctx* ctx, rcppml_rhs_plan* plan, const void* values);
RCPPML_GPU_API void rcppml_hip_rhs_plan_destroy(rcppml_rhs_plan* plan);
RCPPML_GPU_API int rcppml_hip_rhs_plan_info(const rcppml_rhs_plan* plan, double* out11);
RCPPML_GPU_API int rcppml_hip_rhs_planned(rcppml_hip_ctx* ctx, const rcppml_rhs_plan* plan, const void* F, void* B);

/* Per-column CD NNLS -- reference primitives/cpu/nnls_batch.hpp:70-132 (cd_nnls_col_fixed) with the
 * prologues of fused_nnls.hpp:116-123 / nnls_batch.hpp:167-174:
 *   b = B(:,j); if (l1_pre>0) b -= l1_pre; x = zero_init ? 0 : X(:,j); if (warm) b -= G x;
 *   CD(G, b, x, l1_cd, l2_cd, nonneg, maxit, ub_cd, tol); if (ub_post>0) x = min(x, ub_post).
 * B is NOT modified (the residual lives in registers).  G: k x k.
 * sweeps_out (device, ncols ints, may be NULL): sweeps executed per column = the value cd_nnls_col_fixed
 * returns (nnls_batch.hpp:127-131).  With tol = 0 that is maxit on every column, also where the static-sweep kernel
 * RCPPML_CD_AUTO takes for small sides (k <= 64, plain non-negative steps, ncols <= 6 x CUs) leaves early because a sweep
 * moved no coordinate: the sweeps it skips are no-ops, and it reports maxit as the reference does.
 * col_order (device, ncols ints, may be NULL): work order -- slot s of the launch solves column col_order[s]
 * (see rcppml_hip_order_columns).  Columns are independent: any permutation gives identical results. */
RCPPML_GPU_API int rcppml_hip_solve_cd(rcppml_hip_ctx* ctx, int dtype, const void* G, const void* B,
                                       void* X, int k, int64_t ncols, double l1_pre, int warm,
                                       int zero_init, double l1_cd, double l2_cd, int nonneg,
                                       int maxit, double tol, double ub_cd, double ub_post,
                                       int variant, int* sweeps_out, const int* col_order);

/* order = columns sorted by DESCENDING sweeps (counting sort on the device).  Feeding the sweep counts of the
 * previous ALS iteration groups columns that converge together into the same wavefront. */
RCPPML_GPU_API int rcppml_hip_order_columns(rcppml_hip_ctx* ctx, const int* sweeps, int64_t ncols, int* order);

/* Cholesky solve + clip -- reference primitives/cpu/fused_nnls.hpp:185-219:
 *   L = chol(G) once; x = L^-T L^-1 (B(:,j) - l1_pre); clip >= 0 (nonneg); clip <= ub_post. */
RCPPML_GPU_API int rcppml_hip_solve_chol(rcppml_hip_ctx* ctx, int dtype, const void* G,
                                         const void* B, void* X, int k, int64_t ncols,
                                         double l1_pre, int nonneg, double ub_post);

/* Row norms of X (k x c): out[i] = sum_j |X_ij| (norm_type 0), sum_j X_ij^2 (norm_type 1) or sum_j X_ij (norm_type 3);
 * no epsilon, no sqrt -- the distributed harness all-reduces these partial sums. */
RCPPML_GPU_API int rcppml_hip_row_norms(rcppml_hip_ctx* ctx, int dtype, const void* X, int k,
                                        int64_t ncols, int norm_type, void* out);
/* d = (norm_type==1 ? sqrt(s) : s) + 1e-15; X(i,:) /= d_i -- reference
 * nmf/variant_helpers.hpp:286-305.  `sums` as produced by rcppml_hip_row_norms. */
RCPPML_GPU_API int rcppml_hip_apply_scaling(rcppml_hip_ctx* ctx, int dtype, void* X, int k,
                                            int64_t ncols, int norm_type, const void* sums, void* d);

/* extract_scaling (rcppml_hip_row_norms + rcppml_hip_apply_scaling: the same row sums, d and X, bit for bit) and -- when `sweeps` /
 * `order` are not NULL -- rcppml_hip_order_columns(sweeps, ncols, order) for the NEXT solve of this side inside the same three
 * launches instead of five (independent kernels share a launch: the histogram beside the row sums, the scatter beside the scaling).  Reference:
 * nmf/variant_helpers.hpp:286-305 (the work order has no reference counterpart).  `sums`: k values of scratch (the raw row sums). */
RCPPML_GPU_API int rcppml_hip_scale_order(rcppml_hip_ctx* ctx, int dtype, void* X, int k, int64_t ncols, int norm_type,
                                          void* sums, void* d, const int* sweeps, int* order);

/* sum of squares of a length-len vector in fp64 -> out[0] (double, device) -- trace_AtA,
 * reference primitives/primitives.hpp:100-115. */
RCPPML_GPU_API int rcppml_hip_sumsq(rcppml_hip_ctx* ctx, int dtype, const void* x, int64_t len,
                                    double* out);

/* MSE loss by the Gram trick -- reference nmf/fit_cpu.hpp:1710-1753:
 *   cross = sum_{l,i} d_i W_T(i,l) B_w(i,l); recon = sum_ij d_i d_j G_wt(i,j) G_saved(i,j);
 *   out[0] = trAtA[0] - 2 cross + recon; out[1] = cross; out[2] = recon   (double, device). */
RCPPML_GPU_API int rcppml_hip_loss_mse(rcppml_hip_ctx* ctx, int dtype, const double* trAtA,
                                       const void* d, const void* W_T, const void* B_w, int k,
                                       int64_t m, const void* G_wt, const void* G_saved,
                                       double* out);

/* G_wt = W_T W_T^T + eps I (rcppml_hip_gram with l2 = 0) and then rcppml_hip_loss_mse with it, in three launches instead of four (the
 * cross-term partials share the launch of the Gram's final sum);
 * the same G_wt and out[0..2] bit for bit -- reference nmf/fit_cpu.hpp:1729-1753. */
RCPPML_GPU_API int rcppml_hip_gram_loss_mse(rcppml_hip_ctx* ctx, int dtype, const void* W_T, int k, int64_t m, double eps,
                                            const double* trAtA, const void* d, const void* B_w, const void* G_saved,
                                            void* G_wt, double* out);

/* The tail of a half-update in one call.  rcppml_hip_tail_scale_gram = rcppml_hip_scale_order(X, ...) then rcppml_hip_gram(X, eps, l2)
 * -> G (the H side: extract_scaling of H, then its Gram for the W update; nmf/fit_cpu.hpp:645, :715-722);
 * rcppml_hip_tail_scale_gram_loss = rcppml_hip_scale_order(W_T, ...) then rcppml_hip_gram_loss_mse (the W side: extract_scaling of W_T,
 * its Gram and the loss; :893, :1729-1753).  Same results as the separate calls bit for bit.  fp32 with k = 64 runs the scaling pass
 * INSIDE the Gram's partial-tile kernel (the lane that loads an element divides, stores and multiplies it): four and five launches
 * instead of seven and nine; every other shape takes the two calls above. */
RCPPML_GPU_API int rcppml_hip_tail_scale_gram(rcppml_hip_ctx* ctx, int dtype, void* X, int k, int64_t ncols, int norm_type, void* sums,
                                              void* d, const int* sweeps, int* order, double eps, double l2, void* G);
RCPPML_GPU_API int rcppml_hip_tail_scale_gram_loss(rcppml_hip_ctx* ctx, int dtype, void* W_T, int k, int64_t m, int norm_type, void* sums,
                                                   void* d, const int* sweeps, int* order, double eps, const double* trAtA,
                                                   const void* B_w, const void* G_saved, void* G_wt, double* out);

/* The WHOLE plain sparse MSE fit of a SMALL matrix as one persistent kernel on one XCD (kernels_small.hip.h; round 6): nmf_fit<CPU>
 * (nmf/fit_cpu.hpp:444-1855) with fused right-hand side + solve per column (primitives/cpu/fused_nnls.hpp:70-134 CD, :185-219
 * Cholesky + clip), L1 / L2 / upper bounds / non-negativity, row scaling (nmf/variant_helpers.hpp:286-305), Gram-trick loss every
 * iteration (fit_cpu.hpp:1729-1753) and the convergence rule (:1769-1809) evaluated on the device -- no launch per phase, no host
 * round trip per iteration.  The iteration's grid-wide dependencies are barriers inside the kernel among 32 workgroups that all
 * sit on XCD 0 (one L2: a relaxed L2 atomic + an L1 invalidate, 0.8 us; profiles/r06_grid_barrier.txt).
 * rcppml_hip_als_small_eligible: where the kernel PAYS and the plugin takes it -- k <= 16, m + n <= 3072, nnz <= 2^17 (measured:
 * profiles/r06_small_threshold.txt; hawaiibirds is, movielens at k = 32 is not); rcppml_hip_als_small_fit itself accepts k <= 32, nnz <= 2^20, m + n <= 65536.
 * CSC(A) and CSC(A^T) with sorted rows; W (k x m), H (k x n) in / out, d (k) out; trAtA = sum a^2 (device, rcppml_hip_sumsq);
 * iter0: iterations already run by earlier calls on these factors (0 = a fit from its start: iteration 0 then solves without the
 * warm-start correction; > 0 continues a fit -- bench.py's warm-up / timed split); loss_history: max_iter doubles (device, may be NULL); result8 (device): [0] iterations [1] converged [2] train loss [3] last relative
 * change [4] 1 = done, anything else = the kernel gave up at a barrier (its workgroups did not all land on one XCD): W / H are then
 * partly overwritten and the caller must restart on the multi-launch ops; [5..7] workgroup 0's 100 MHz clock ticks inside the launch:
 * fused half-updates, waiting at barriers, whole kernel (bench.py --config c1 `inside_the_kernel`). */
RCPPML_GPU_API int rcppml_hip_als_small_eligible(int m, int n, int64_t nnz, int k);
RCPPML_GPU_API int rcppml_hip_als_small_fit(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx, const void* values,
                                            const int* t_col_ptr, const int* t_row_idx, const void* t_values, int m, int n, int64_t nnz,
                                            int k, void* W, void* H, void* d, const double* trAtA, double L1_H, double L1_W, double L2_H,
                                            double L2_W, double ub_H, double ub_W, int nonneg_H, int nonneg_W, int norm_type,
                                            int solver_mode, int cd_maxit, double cd_tol, int max_iter, double tol, int patience,
                                            int iter0, double* loss_history, double* result8);

/* Explicit-mask per-column NNLS -- reference nmf/masked_nnls.hpp:96-154 / 177-242.
 * A and mask share shape (rows x ncols, CSC; mask nonzero = masked; mask values not needed). */
RCPPML_GPU_API int rcppml_hip_solve_masked(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr,
                                           const int* row_idx, const void* values,
                                           const int* mask_p, const int* mask_i, int64_t ncols,
                                           const void* F, const void* G_full, void* X, int k,
                                           double l1, double l2, int nonneg, int cd_maxit,
                                           double cd_tol, int solver_mode, int warm);
/* Over unmasked NONZEROS, with p = sum_f d_f W_T(f,i) H(f,j):  out[0] = sum (a - p)^2 (reference
 * nmf/masked_nnls.hpp:250-282), out[1] = sum p^2.  mask_p may be NULL (no mask: all nonzeros).
 * out: 2 doubles, device. */
RCPPML_GPU_API int rcppml_hip_loss_nonzeros(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr,
                                            const int* row_idx, const void* values,
                                            const int* mask_p, const int* mask_i, int64_t ncols,
                                            const void* W_T, const void* d, const void* H, int k,
                                            double* out);
/* The same pass with the per-element term of the configured loss: out[0] = sum over the unmasked nonzeros of
 * compute_loss(a, p, loss) (math/loss.hpp:512-536) -- the loss of a fit that has BOTH an explicit mask and a distribution loss
 * (fit_cpu.hpp:1685-1690 -> nmf/masked_nnls.hpp:250-282, :277).  As in the reference the term is evaluated with theta = 0 (masked_loss
 * passes no dispersion) and without the robust modifier.  loss_type 0 (MSE) or 4..8; out: 2 doubles, device (out[1] = sum p^2). */
RCPPML_GPU_API int rcppml_hip_loss_masked(rcppml_hip_ctx* ctx, int dtype, int loss_type, double tweedie_power,
                                          const int* col_ptr, const int* row_idx, const void* values,
                                          const int* mask_p, const int* mask_i, int64_t ncols,
                                          const void* W_T, const void* d, const void* H, int k, double* out);

/* Cross-validation (reference nmf/fit_cv.hpp, nmf/cv_detail.hpp, nmf/speckled_cv.hpp).  The held-out
 * set is the lazy speckled mask  SplitMix64::hash(seed, i, j) < UINT64_MAX / floor(1 / holdout_fraction)  with
 * seed = (uint32) cv_seed (0 -> 12345) and (i, j) the coordinates in A (rng/rng.hpp:129-170); no mask matrix exists.
 * rcppml_hip_solve_cv: one CV half-update over the columns of the CSC handed in (A for H, A^T with transposed = 1 for
 *   W; nrows = its row count): b = sum over the column's TRAIN nonzeros, G_local = G - sum over its TEST rows f f^T
 *   (mask_zeros = 1: held-out nonzeros only; 0: every held-out row, zeros included), then Cholesky+clip (solver_mode 1,
 *   L1 subtracted from b) or CD (solver_mode 0: L1 inside, cd_maxit sweeps, no tolerance) started from the current X
 *   without a warm-start correction -- fit_cv.hpp:420-478,591-830.  k <= 128 (above 64: kernels_wide.hip.h).
 * rcppml_hip_cv_test_error: out2[0] = sum of squared errors, out2[1] = count over the held-out entries of A
 *   (prediction W diag(d) H; fit_cv.hpp:1444-1494). */
RCPPML_GPU_API int rcppml_hip_solve_cv(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx,
                                       const void* values, int64_t ncols, int nrows, const void* F, const void* G, void* X,
                                       int k, double holdout_fraction, unsigned long long cv_seed, int mask_zeros,
                                       int transposed, double l1, int nonneg, int cd_maxit, int solver_mode);
/* The user mask of a CV fit (see rcppml_gpu_nmf_cv_masked_ex): device pointers to the pattern CSC of the mask (rows x cols of A) and of
 * its transpose; they must stay valid until the mask is cleared (all four NULL).  While set, rcppml_hip_solve_cv,
 * rcppml_hip_solve_cv_irls and rcppml_hip_cv_irls_loss exclude its entries as the reference does (rcppml_hip_cv_test_error does not: with
 * a mask both losses come from rcppml_hip_cv_irls_loss, loss_type 0). */
RCPPML_GPU_API int rcppml_hip_ctx_set_cv_mask(rcppml_hip_ctx* ctx, const int* mask_p, const int* mask_i, const int* maskT_p,
                                              const int* maskT_i);
RCPPML_GPU_API int rcppml_hip_cv_test_error(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx,
                                            const void* values, int64_t ncols, int nrows, const void* W_T, const void* d,
                                            const void* H, int k, double holdout_fraction, unsigned long long cv_seed,
                                            int mask_zeros, double* out2);

/* Graph (Laplacian) regularisation -- reference features/graph_reg.hpp:38-50 at its fused-path place
 * (nmf/fit_cpu.hpp:508-509,741-742):  G += lambda * (X L) X^T  for the CURRENT factor X (k x ncols) and a sparse
 * ncols x ncols Laplacian L in CSC (device).  X L is formed by the SpMM kernel, the k x k product by a blocked reduction
 * with a fixed summation order.  k <= 128. */
RCPPML_GPU_API int rcppml_hip_apply_graph_reg(rcppml_hip_ctx* ctx, int dtype, void* G, const int* lap_p, const int* lap_i,
                                              const void* lap_x, const void* X, int k, int64_t ncols, double lambda);

/* Y = diag(d) X for a k x ncols factor (variant_helpers.hpp:265-272 apply_scaling): W diag(d) of the projective H
 * update  H = (diag(d) W_T) A  (nmf/fit_cpu.hpp:462-472, variant_helpers.hpp:308-325). */
RCPPML_GPU_API int rcppml_hip_mul_rows(rcppml_hip_ctx* ctx, int dtype, const void* X, int k, int64_t ncols, const void* d, void* Y);

/* Y = X + alpha * T elementwise (n entries) and G(i,i) += v: the two device-side pieces of target regularisation
 * (nmf/variant_helpers.hpp:107-111: G.diagonal() += lambda; B += lambda * target). */
RCPPML_GPU_API int rcppml_hip_axpy(rcppml_hip_ctx* ctx, int dtype, const void* X, const void* T, double alpha, int64_t n, void* Y);
RCPPML_GPU_API int rcppml_hip_add_diag(rcppml_hip_ctx* ctx, int dtype, void* G, int k, double v);
/* X = min(X, ub) over n entries (features/bounds.hpp apply_upper_bound; nmf/fit_cpu.hpp:636-637, 884-885). */
RCPPML_GPU_API int rcppml_hip_clip_upper(rcppml_hip_ctx* ctx, int dtype, void* X, int64_t n, double ub);

/* k x k feature layer, fused-path placement of nmf/fit_cpu.hpp:505-511,636-639 / :738-745,884-887:
 * rcppml_hip_apply_l21: G(i,i) += lambda / ||X.row(i)||_2 for rows with norm > 1e-10 (features/L21.hpp:38-51); X is the
 *   CURRENT factor (k x ncols), applied to the Gram before the solve.
 * rcppml_hip_angular_posthoc: X <- max(0, X - lambda * diag(norms) * offdiag(Xh Xh^T) Xh), Xh = rows of X scaled to unit
 *   norm (features/angular.hpp:67-103); applied after the solve and the upper bound, before scaling.  k <= 128. */
RCPPML_GPU_API int rcppml_hip_apply_l21(rcppml_hip_ctx* ctx, int dtype, void* G, const void* X, int k, int64_t ncols,
                                        double lambda);
RCPPML_GPU_API int rcppml_hip_angular_posthoc(rcppml_hip_ctx* ctx, int dtype, void* X, int k, int64_t ncols, double lambda);

/* NB (negative-binomial) IRLS half-update -- reference primitives/cpu/nnls_batch_irls.hpp:465-520,202-329 with the NB
 * weight of math/loss.hpp:248-256: X = 0; per column up to irls_max_iter passes of
 *   w_i = min(r/(mu(r+mu)), 1e6) at the column's nonzeros (mu = F(:,i).x, in fp64), G_w = G_base + F_nz diag(w-1) F_nz^T
 *   (+ l2 on the diagonal), b_w = F_nz (w o a), b = b_w - G_w x, CD(G_w, b, x, L1 inside, cd_maxit sweeps, no tolerance),
 *   stop when max |dx|/(|x_old|+1e-12) < irls_tol.
 * theta_row: NB size indexed by the nonzero's row (H side) or theta_col: indexed by the column (W side over A^T);
 * exactly one is non-NULL.  k <= 128 (above 64: one wave per column with two features per lane, kernels_wide.hip.h).
 * The tolerance-free sweeps end early at the iterate's floating-point fixed point (a whole sweep that changes no coordinate). */
RCPPML_GPU_API int rcppml_hip_solve_irls_nb(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx,
                                            const void* values, int64_t ncols, const void* F, const void* G_base,
                                            void* X, int k, double l1, double l2, int nonneg, int cd_maxit,
                                            int irls_max_iter, double irls_tol, const void* theta_row,
                                            const void* theta_col);
/* Generic forms: loss_type = the reference's LossType (math/loss.hpp:36-47), implemented: 5 = NB, 4 = GP, 6 = Gamma,
 * 7 = inverse Gaussian, 8 = Tweedie (loss_param = the variance power p; ignored otherwise).  The GP loss updates W and H
 * with the KL weight 1/max(mu, 1e-4) (nmf/fit_cpu.hpp:568-574: "GP strategy: use KL weights for W/H updates") and
 * evaluates the GP likelihood (math/loss.hpp:382-398) with theta_row (zeros for dispersion = "none": Poisson /
 * KL-divergence NMF); 6-8 use the power-variance weight min(1/mu^p, 1e6) (:270-278) and the deviance terms (:439-505).
 * theta pointers are read by NB only (pass NULL otherwise).  The plugin implements 4 and 6-8 for dispersion = "none".
 * robust_delta > 0 multiplies every weight by the Huber modifier of the Pearson residual (math/loss.hpp:294-303,
 * nnls_batch_irls.hpp:95-120) and makes the loss the Huber rho of that residual (:549-607); with it loss_type 0 (MSE,
 * distribution weight 1) is accepted too -- the reference routes robust MSE through the IRLS path. */
RCPPML_GPU_API int rcppml_hip_solve_irls(rcppml_hip_ctx* ctx, int dtype, int loss_type, const int* col_ptr,
                                         const int* row_idx, const void* values, int64_t ncols, const void* F,
                                         const void* G_base, void* X, int k, double l1, double l2, int nonneg,
                                         int cd_maxit, int irls_max_iter, double irls_tol, const void* theta_row,
                                         const void* theta_col, double loss_param, double robust_delta);
RCPPML_GPU_API int rcppml_hip_irls_loss(rcppml_hip_ctx* ctx, int dtype, int loss_type, const int* col_ptr,
                                        const int* row_idx, const void* values, int64_t ncols, const void* W_T,
                                        const void* d, const void* H, const void* theta_row, int k, double loss_param,
                                        double robust_delta, double* out);
/* Dense-input right-hand sides (reference primitives::rhs<CPU> on a dense A and detail::rhs_transpose,
 * nmf/fit_cpu.hpp:547-549 / :783): transposed = 0: B (k x n) = F (k x m) A;  1: B (k x m) = F (k x n) A^T.
 * A column-major m x n on the device; F, B column-major with leading dimension k, k <= 128.  Hand-written skinny MFMA GEMMs
 * (fp32 32x32x2 tiles, fp64 16x16x4 tiles) that stream A once; no BLAS library. */
RCPPML_GPU_API int rcppml_hip_rhs_dense(rcppml_hip_ctx* ctx, int dtype, const void* A, int64_t m, int64_t n,
                                        int transposed, const void* F, int k, void* B);
/* The launch geometry rcppml_hip_rhs_dense uses for this problem (host arithmetic, no device needed; what
 * rcppml_hip_rhs_plan_info is to the sparse plans): out[0] = blocks of output columns, out[1] = slices the reduction is split
 * into (1: B is written directly; > 1: per-slice partials summed in slice order), out[2] = reduction indices per slice (a
 * multiple of the 32- (forward) or 16-index (backward) chunk; the last slice may hold fewer), out[3] = the kernels' row-tile
 * template parameter (fp32: 1..4 tiles of 32 factor rows; fp64: 1, 2, 4 or 8 tiles of 16).  All zero for an empty problem. */
RCPPML_GPU_API int rcppml_hip_rhs_dense_geometry(int dtype, int64_t m, int64_t n, int k, int transposed, int64_t* out);
/* Same decoder on a byte buffer in host memory, into caller-allocated device arrays (layer 2; what the parity tests
 * call).  Format restated from streampress/sparsepress_v2.hpp:897-1090, codec/rans.hpp:128-247, codec/varint.hpp:43-52.
 * rcppml_hip_spz_info parses the 128-byte header only (host).  Both return the out_status codes above. */
RCPPML_GPU_API int rcppml_hip_spz_info(const void* file_bytes, uint64_t size, int* m, int* n, int64_t* nnz, int* value_type);
RCPPML_GPU_API int rcppml_hip_spz_decode(rcppml_hip_ctx* ctx, const void* file_bytes, uint64_t size, int* d_col_ptr,
                                         int* d_row_idx, double* d_values);

/* Dispersion estimators of the other IRLS losses, per ROW of A (takes CSC(A^T), nnz = its nonzero count):
 *   loss_type 4        GP theta by the auxiliary-function (MM) update, five inner passes -- reference
 *                      nmf/fit_cpu.hpp:914-1008 (PER_ROW / GLOBAL, sparse branch); hi = gp_theta_max, lo unused;
 *   loss_type 6 / 7 / 8  Gamma / inverse-Gaussian / Tweedie phi by the Pearson method of moments over the positive
 *                      nonzeros, clamped to [lo, hi] -- nmf/fit_cpu.hpp:1561-1670; power = Tweedie variance power.
 * mode 2 = PER_ROW, 1 = GLOBAL (GP: mean of the per-row values; phi: the median sorted[m/2]).  theta (m) is updated in
 * place (rows without usable nonzeros keep their value). */
RCPPML_GPU_API int rcppml_hip_dispersion_update(rcppml_hip_ctx* ctx, int dtype, int loss_type, int mode,
                                                const int* t_col_ptr, const int* t_row_idx, const void* t_values,
                                                int64_t m, int64_t nnz, const void* W_T, const void* d, const void* H,
                                                int64_t n, int k, double power, double lo, double hi, void* theta);
/* GLOBAL dispersion: x[0..m) <- mean(x) (stat 0; fit_cpu.hpp:1005-1008) or <- sorted(x)[m/2] (stat 1: the reference's
 * nth_element at m/2; NB fit_cpu.hpp:1257-1262, phi :1664-1669). */
RCPPML_GPU_API int rcppml_hip_vec_global(rcppml_hip_ctx* ctx, int dtype, int stat, void* x, int64_t m);
/* NB size (r) per ROW of A by the method of moments -- reference nmf/fit_cpu.hpp:1094-1265 (PER_ROW branch, sparse):
 * r_i = clamp(S mu^2 / (S (y-mu)^2 - S mu), r_min, r_max), else r_max.  Takes CSC(A^T); W_T k x m, H k x n. */
RCPPML_GPU_API int rcppml_hip_nb_size_update(rcppml_hip_ctx* ctx, int dtype, const int* t_col_ptr,
                                             const int* t_row_idx, const void* t_values, int64_t m, const void* W_T,
                                             const void* d, const void* H, int64_t n, int k, double r_min,
                                             double r_max, void* nb_size);
/* The two calls above and below in one pass over CSC(A^T) (PER_ROW dispersion, no robust modifier): nb_size updated as by
 * rcppml_hip_nb_size_update, then out[0] = the NB negative log-likelihood with the UPDATED sizes, as rcppml_hip_nb_loss returns it
 * (the order of the reference's fit loop, nmf/fit_cpu.hpp:1094-1265 then :1684-1753 / explicit_loss.hpp:53-77).  The predictions of
 * the first pass are parked (nnz Scalars of context scratch) and the likelihood terms are evaluated from them: one gather of
 * factor rows per nonzero instead of two, lgamma(r_i) once per row.  nnz = t_col_ptr[m]. */
RCPPML_GPU_API int rcppml_hip_nb_size_update_loss(rcppml_hip_ctx* ctx, int dtype, const int* t_col_ptr,
                                                  const int* t_row_idx, const void* t_values, int64_t m, int64_t nnz,
                                                  const void* W_T, const void* d, const void* H, int64_t n, int k,
                                                  double r_min, double r_max, void* nb_size, double* out);
/* out[0] = NB negative log-likelihood over the NONZEROS of A with per-row size -- reference nmf/explicit_loss.hpp:53-77,
 * math/loss.hpp:415-426. */
RCPPML_GPU_API int rcppml_hip_nb_loss(rcppml_hip_ctx* ctx, int dtype, const int* col_ptr, const int* row_idx,
                                      const void* values, int64_t ncols, const void* W_T, const void* d, const void* H,
                                      const void* theta_row, int k, double* out);

/* Cross-validation with the IRLS losses -- reference nmf/cv_detail.hpp:101-292 (irls_solve_col_cv / irls_solve_row_cv), callers
 * nmf/fit_cv.hpp:446-456, :670-689.  Per column of the CSC (H side: A, F = W_T; W side: A^T with transposed = 1, F = H; the speckled
 * mask SplitMix64::hash(seed, i, j) < UINT64_MAX / floor(1 / fraction) is always asked in the coordinates of A), up to irls_max_iter
 * passes of:  G_w = sum over the TRAINING entries of w f f^T + G_add + 1e-15 I,  b_w = sum (w a) f,  x <- CD(G_w, b_w, x; L1
 * inside, cd_maxit sweeps, no tolerance) or Cholesky + clip, started from the current column WITHOUT a residual correction of
 * b_w, until max |dx| / (|x_old| + 1e-12) < irls_tol.  Training entries: the nonzeros that are not held out (mask_zeros = 1) or
 * every row that is not held out, zeros included (0).  The weight is the reference's compute_irls_weight(residual, predicted,
 * loss) with its DEFAULT observed = 0 and theta = 0: NB / Gamma / inverse Gaussian / Tweedie distribution weights at theta 0,
 * GP = irls_weight_gp(0, mu, 0, blend 1) (math/loss.hpp:197-229; not the KL weight of the non-CV fit), times the Huber
 * modifier when robust_delta > 0.  G_add (k x k, may be NULL): the additive CV features (L2, graph, L21).  k <= 128. */
RCPPML_GPU_API int rcppml_hip_solve_cv_irls(rcppml_hip_ctx* ctx, int dtype, int loss_type, const int* col_ptr, const int* row_idx,
                                            const void* values, int64_t ncols, int nrows, const void* F, const void* G_add, void* X,
                                            int k, double holdout_fraction, unsigned long long cv_seed, int mask_zeros,
                                            int transposed, double l1, int nonneg, int cd_maxit, int solver_mode, int irls_max_iter,
                                            double irls_tol, double loss_param, double robust_delta);
/* out4 = {train sum, n_train, test sum, n_test} of compute_loss(value, prediction, loss, theta) (math/loss.hpp:511-535; loss_type 0
 * = squared error) over the entries of A -- the nonzeros (mask_zeros = 1) or every entry -- split by the speckled mask; theta_row
 * (per row, may be NULL) is read by GP only.  Reference nmf/fit_cv.hpp:1377-1443. */
RCPPML_GPU_API int rcppml_hip_cv_irls_loss(rcppml_hip_ctx* ctx, int dtype, int loss_type, const int* col_ptr, const int* row_idx,
                                           const void* values, int64_t ncols, int nrows, const void* W_T, const void* d,
                                           const void* H, const void* theta_row, int k, double holdout_fraction,
                                           unsigned long long cv_seed, int mask_zeros, double loss_param, double* out4);
/* GP theta per row by the MM update (five inner passes) over the TRAINING entries only -- reference nmf/fit_cv.hpp:866-961: held-out
 * nonzeros are skipped and the held-out pairs' predictions (zeros included) are taken out of sum_s.  Takes CSC(A^T) (nnz = its
 * nonzero count).  mode 2 = PER_ROW, 1 = GLOBAL (mean).  holdout_fraction 0: the non-CV update. */
RCPPML_GPU_API int rcppml_hip_cv_gp_theta_update(rcppml_hip_ctx* ctx, int dtype, int mode, const int* t_col_ptr, const int* t_row_idx,
                                                 const void* t_values, int64_t m, int64_t nnz, const void* W_T, const void* d,
                                                 const void* H, int64_t n, int k, double holdout_fraction,
                                                 unsigned long long cv_seed, double theta_max, void* theta);

/* Factor graphs (rcppml_amd/csrc/ops_graph.hip, kernels_graph.hip.h).  Build-defined: R has no hook for them.  The specification is the
 * reference's multi-layer fit, inst/include/FactorNet/graph/fit.hpp:100-194 (effective_input) and :264-375 (fit_deep).  fp64.
 *
 * rcppml_hip_graph_assemble: the effective input X (n x c, column-major, device) of a deeper layer from n_branches (1..8) upstream
 *   factors H[b] (k[b] x n, leading dimension k[b], device pointers in a HOST array) and an optional condition block Z (p x n,
 *   column-major; NULL / p = 0: none).  mode 0 (concat; one branch = the plain chain): X = [t(H_0) | t(H_1) | ... | t(Z)],
 *   c = sum k[b] + p.  mode 1 (add; all k[b] equal): X = [t(H_0 + H_1 + ...) | t(Z)], c = k[0] + p, summed in branch order.  One
 *   launch, a transposing gather through an LDS tile; no atomics, exact.
 * rcppml_hip_graph_layer_loss: out[0] (double, device) = scale * sum_ij (X_ij - sum_f W_T[f, i] d_f H[f, j])^2 for a dense X
 *   (rows x c, column-major), W_T k x rows, d k, H k x c, k <= 128.  Two launches; the summation order depends on (rows, c, k)
 *   only: bitwise-repeatable. */
RCPPML_GPU_API int rcppml_hip_graph_assemble(rcppml_hip_ctx* ctx, int dtype, int mode, int n_branches, const void* const* H,
                                             const int* k, int64_t n, const void* Z, int p, void* X);
RCPPML_GPU_API int rcppml_hip_graph_layer_loss(rcppml_hip_ctx* ctx, int dtype, const void* X, int64_t rows, int c, const void* W_T,
                                               const void* d, const void* H, int k, double scale, double* out);

/* rcppml_gpu_factor_net_fit_ex: fit_deep on the device.  Every layer's factors stay on the device between the upload and the final
 * download; the first layer's matrix, its transpose and the right-hand-side plans are built once per call; the host reads one
 * scalar (the summed loss) per outer iteration, and one per warm-up iteration when *tol > 0 (the fit's own convergence rule).
 *
 * The first layer's data: a host CSC (col_ptr, row_idx, values, *nnz; row indices strictly increasing within a column) or a
 * column-major *m x *n dense array, exactly one of the two.
 * The graph, layers in topological order, layer i = 0 .. *n_layers - 1 (1 .. 64):
 *   rank[i]                        1 .. 128 (1 .. 64 with the Cholesky solver: the fp64 Cholesky solve)
 *   src_kind[i]                    0 input (the data), 1 layer, 2 concat, 3 add
 *   branch_ptr (n_layers + 1), branch_idx   the upstream layers of layer i: branch_idx[branch_ptr[i] .. branch_ptr[i + 1]), each < i;
 *                                  none for kind 0, one for kind 1, 2 .. 8 for kinds 2 and 3 (add: equal ranks).  All branches of a layer
 *                                  have the same number of H columns.
 *   cond_p[i], cond_Z              rows p of the layer's condition block (0: none; kinds 1 .. 3 only) and the blocks (p x rows_i,
 *                                  column-major) packed in layer order
 *   The layer factorises X_i (rows_i x cols_i) ~ W_i diag(d_i) H_i:  kind 0: m x n;  otherwise rows_i = the branches' H columns and
 *   cols_i = sum of the branch ranks (concat, layer) or the common rank (add), plus p.
 *   L1, L2, upper_bound, nonneg    2 * n_layers values each: [2 i] the W side, [2 i + 1] the H side of layer i
 * *max_iter >= 1, *tol, *seed (0 means 42), *solver_mode (0 CD, 1 Cholesky + clip), *norm_type (0 L1, 1 L2, 2 none), *cd_maxit, *cd_tol.
 * *start: 0 = the reference's warm-up pass (per layer: factors from one SplitMix64 stream seeded seed + i, W_T then H, and
 *   min(10, *max_iter) iterations of the plain MSE fit with *tol and patience 5); 1 = W, d, H hold every layer's state on entry and
 *   the warm-up is skipped.
 * W, d, H (in with *start = 1, out always): per layer W_T (rank x rows_i), d (rank), H (rank x cols_i), column-major, packed in
 *   layer order.  out_layer_loss (n_layers): the layers' mean squared reconstruction errors of the last outer iteration.
 * *out_loss reproduces the reference's total_loss: the previous iteration's summed loss when the loop stops on
 *   |prev - cur| / (|prev| + 1e-15) < *tol, the last one when it runs out (fit.hpp:345-359).
 * out_counts (2 ints, may be NULL): device-op calls and own kernel launches of ONE outer iteration.
 * Refused (*out_status = -1, reason in rcppml_gpu_last_error, no output written): a null pointer; a malformed graph, CSC or shape;
 *   a non-finite value; a rank above 128 (64 with Cholesky); not enough free device memory (the message gives the byte count); no
 *   HIP device. */
RCPPML_GPU_API void rcppml_gpu_factor_net_fit_ex(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
        const double* dense, int* m, int* n, int* n_layers, const int* rank, const int* src_kind, const int* branch_ptr,
        const int* branch_idx, const int* cond_p, const double* cond_Z, const double* L1, const double* L2,
        const double* upper_bound, const int* nonneg, int* max_iter, double* tol, int* seed, int* solver_mode, int* norm_type,
        int* cd_maxit, double* cd_tol, int* start, double* W, double* d, double* H, double* out_layer_loss, int* out_iter,
        int* out_converged, double* out_loss, int* out_counts, int* out_status);

/* Column similarities and factor matching (rcppml_amd/csrc/ops_similarity.hip): the compute side of the reference's cosine(),
 * bipartiteMatch() and align() (R/cosine.R, R/bipartiteMatch.R, R/nmf_methods.R:261-271).  Build-defined: R has no hook for these
 * entries and no GPU form of any of them.  fp64.  No atomics: every value has one fixed order of operations, every product and sum is
 * rounded on its own (no FMA contraction), so results are bitwise-repeatable and do not depend on the launch.  A column of zero norm
 * (zero centred norm for the correlation) has similarity 0 to every column, itself included.
 * Refused (*out_status = -1, reason in rcppml_gpu_last_error, no output written): a null pointer, a size below 1, a malformed CSC
 * (row indices strictly increasing within a column), a non-finite value, kx or ky above 128, a method outside {0, 1}, groups < 0, not
 * enough free device memory (the message gives the byte count), no HIP device (the two device entries).
 *
 * rcppml_gpu_cosine_sparse_ex: out_C (*nx x *ny, column-major) with C[i, j] = <x_i, y_j> / (|x_i| |y_j|) for the columns of X (*m x
 * *nx) and Y (*m x *ny), both CSC.  y_col_ptr NULL: Y = X (the y arguments and *ny are not read, the result is *nx x *nx and exactly
 * symmetric: C[i, j] and C[j, i] are the same chain of operations).  No dense copy of X or Y exists on either side.  <x_i, y_j>: the
 * products of the rows both columns store, added in ascending row order starting from 0; |x|: the squares of a column added in
 * ascending row order, then the square root; C = dot / (|x_i| * |y_j|), 0 where that product is 0.  Sums of squares above the fp64
 * range, or norm products below it, are the caller's to avoid.  *groups: the workgroups of the main kernel, 0 (or NULL) for the
 * default launch; a test switch, the result does not depend on it.  out_launches (may be NULL): kernels launched, the transpose's
 * own excluded.  out_ms (2 doubles, may be NULL): device time from the end of the upload to the last kernel, and the time of the
 * download of C, in milliseconds.  Device memory: 8 nx ny for C, three times the CSC of X, the CSC of Y, 4 m (ceil(nx / T) + 1).
 *
 * rcppml_gpu_cosine_geometry: out[0] = T, the columns of X one wavefront keeps in LDS at a time; out[1] = the wavefronts of a
 * workgroup; out[2] = the workgroups of the default launch before it is capped by the work (one per CU; 0 without a device).
 * Returns 0 (-1 for a null pointer); needs no device for out[0] and out[1].
 *
 * rcppml_gpu_cosine_dense_ex: W holds *reps matrices *m x *kx, R one matrix *m x *ky, all column-major; out holds *reps matrices
 * *kx x *ky column-major, out[q][a, b] = the similarity of column a of W_q and column b of R.  *method 0: cosine.  *method 1:
 * Pearson correlation: the column means first (lane l of a wavefront adds rows l, l + 64, ..., then a butterfly over the 64
 * partials, / m), then the centred dot products and the centred norms; never sum(xy) - m mean(x) mean(y).  Norms: the same lane
 * and butterfly order.  Dot products: rows in chunks of 256 ceil(ceil(m / 256) / 64) rows, ascending inside a chunk, the chunk
 * partials added in chunk order.  A replicate's result does not depend on the other replicates of the stack.  out_launches: 3.
 *
 * rcppml_gpu_bipartite_match_ex: host only, no device work.  cost: *batch matrices *nr x *nc, row-major; negative entries count as 0
 * (R/bipartiteMatch.R:22-25).  Minimum-cost assignment by shortest augmenting paths with dual potentials (Jonker-Volgenant /
 * Hungarian), O(min(nr, nc)^2 max(nr, nc)); rows enter in order and every scan keeps its first minimum, so equal inputs give equal
 * assignments.  out_assignment (*batch x *nr): the column matched to each row, 0-based, -1 for a row left unmatched (nr > nc);
 * out_cost (*batch): the matched entries added in row order. */
RCPPML_GPU_API void rcppml_gpu_cosine_sparse_ex(const int* x_col_ptr, const int* x_row_idx, const double* x_values, int* x_nnz,
        const int* y_col_ptr, const int* y_row_idx, const double* y_values, int* y_nnz, int* m, int* nx, int* ny, int* groups,
        double* out_C, int* out_launches, double* out_ms, int* out_status);
RCPPML_GPU_API int rcppml_gpu_cosine_geometry(int64_t* out);
RCPPML_GPU_API void rcppml_gpu_cosine_dense_ex(const double* W, const double* R, int* m, int* kx, int* ky, int* reps, int* method,
        double* out, int* out_launches, int* out_status);
RCPPML_GPU_API void rcppml_gpu_bipartite_match_ex(const double* cost, int* nr, int* nc, int* batch, int* out_assignment,
        double* out_cost, int* out_status);

#ifdef __cplusplus
}
#endif
#endif /* RCPPML_GPU_H */
