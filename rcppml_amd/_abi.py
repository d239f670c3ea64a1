"""ctypes binding of rcppml_amd/lib/RcppML_gpu.so (C ABI declared in include/rcppml_gpu.h).

This is the ONLY compute backend of the package: there is no CPU or PyTorch fallback.  If the
shared library is missing or cannot be loaded, importing the symbols raises immediately.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RCPPML_GPU_LIB_PATH") or os.path.join(_HERE, "lib", "RcppML_gpu.so")
_lib = None

F32, F64 = 0, 1
CD_AUTO, CD_LANE, CD_WAVE, CD_GROUP, CD_MFMA, CD_MFMA16, CD_LMF = 0, 1, 2, 5, 6, 7, 8
# rcppml_hip_ctx_set_option
OPT_CD_COUNT_NOOP, OPT_CD_LMF_LANE_GROUPS, OPT_CD_LMF_WAVES_PER_SIMD, OPT_CD_NO_LMF, OPT_IRLS_COLUMNS_PER_WAVE, OPT_SMALL_GIVE_UP = 1, 2, 3, 4, 5, 6
OPT_CD_PLACED, OPT_CD_ASSUME_CUS = 7, 8          # launch form of the 32-column MFMA solve (0 auto, 1 always placed, 2 never); test switch
OPT_CD_PRIO = 9                                  # wave priority modes of the fp32 MFMA solves: 32-column mode + 8 x 16-column mode
CD_PRIO_MODES = (0, 1, 2, 3, 4)                  # none; static younger / older round boosted; dynamic scalar step / MFMAs boosted
CD_PRIO_DEFAULT = 3                              # RCPPML_CD_PRIO_DEFAULT: what a new context runs


def cd_prio_value(h_mode, w_mode):
    """The RCPPML_OPT_CD_PRIO value of a pair of modes; anything but CD_PRIO_MODES is refused (as the library refuses it)."""
    if h_mode not in CD_PRIO_MODES or w_mode not in CD_PRIO_MODES:
        raise ValueError("CD priority modes are 0..4, got %r / %r" % (h_mode, w_mode))
    return h_mode + 8 * w_mode


def cd_prio_valid(value):
    return isinstance(value, int) and value >= 0 and (value & 7) in CD_PRIO_MODES and (value >> 3) in CD_PRIO_MODES

# Every symbol include/rcppml_gpu.h declares (tests check the library exports all of them).
EXPORTED_SYMBOLS = [
    "rcppml_gpu_detect", "rcppml_gpu_nmf_unified_float", "rcppml_gpu_nmf_unified_double", "rcppml_gpu_nmf_ex",
    "rcppml_gpu_nmf_cv_unified_float", "rcppml_gpu_nmf_cv_unified_double", "rcppml_gpu_nmf_cv_ex", "rcppml_gpu_nmf_cv_irls_ex", "rcppml_gpu_nmf_cv_masked_ex", "rcppml_hip_ctx_set_cv_mask", "rcppml_gpu_nmf_zerocopy_double",
    "rcppml_gpu_nnls_double", "rcppml_gpu_evaluate_mse_double", "rcppml_gpu_nmf_profile_double", "rcppml_gpu_last_error",
    "rcppml_hip_ctx_create", "rcppml_hip_ctx_destroy", "rcppml_hip_ctx_sync", "rcppml_hip_ctx_stats", "rcppml_hip_ctx_irls_stats", "rcppml_hip_ctx_irls_sweep_stats", "rcppml_hip_ctx_cd_step_stats", "rcppml_hip_ctx_set_option", "rcppml_hip_transpose_csc", "rcppml_hip_transpose_csc_sort", "rcppml_hip_transpose_csc_gather", "rcppml_hip_cast", "rcppml_hip_gram", "rcppml_hip_rhs",
    "rcppml_hip_solve_cd", "rcppml_hip_order_columns", "rcppml_hip_solve_chol", "rcppml_hip_row_norms", "rcppml_hip_apply_scaling",
    "rcppml_hip_sumsq", "rcppml_hip_loss_mse", "rcppml_hip_solve_masked", "rcppml_hip_loss_nonzeros", "rcppml_hip_loss_masked",
    "rcppml_hip_solve_irls_nb", "rcppml_hip_nb_size_update", "rcppml_hip_nb_size_update_loss", "rcppml_hip_nb_loss", "rcppml_hip_solve_irls", "rcppml_hip_rhs_plan_kind", "rcppml_hip_irls_loss", "rcppml_hip_apply_l21", "rcppml_hip_angular_posthoc", "rcppml_hip_solve_cv", "rcppml_hip_cv_test_error", "rcppml_hip_solve_cv_irls", "rcppml_hip_cv_irls_loss", "rcppml_hip_cv_gp_theta_update", "rcppml_hip_mul_rows", "rcppml_hip_apply_graph_reg", "rcppml_hip_dispersion_update", "rcppml_hip_vec_global", "rcppml_hip_spz_info", "rcppml_hip_spz_decode",
    "rcppml_sp_read_gpu", "rcppml_sp_free_gpu", "rcppml_hip_rhs_dense", "rcppml_hip_rhs_dense_geometry", "rcppml_gpu_nmf_dense_unified_float",
    "rcppml_gpu_nmf_dense_unified_double",
    "rcppml_hip_rhs_plan_create", "rcppml_hip_rhs_plan_create_indices", "rcppml_hip_rhs_plan_set_values", "rcppml_hip_rhs_plan_destroy", "rcppml_hip_rhs_plan_info", "rcppml_hip_rhs_planned",
    "rcppml_gpu_nmf_target", "rcppml_hip_axpy", "rcppml_hip_add_diag", "rcppml_hip_clip_upper",
    "rcppml_hip_scale_order", "rcppml_hip_gram_loss_mse", "rcppml_hip_tail_scale_gram", "rcppml_hip_tail_scale_gram_loss",
    "rcppml_hip_als_small_eligible", "rcppml_hip_als_small_fit",
    "rcppml_gpu_bipartition_double", "rcppml_gpu_dclust_double", "rcppml_gpu_bipartition_ex", "rcppml_gpu_dclust_ex",
    "rcppml_gpu_svd_pca_double", "rcppml_gpu_svd_pca_float", "rcppml_gpu_svd_pca_dense_double", "rcppml_gpu_svd_pca_dense_float",
    "rcppml_gpu_svd_cv_ex", "rcppml_gpu_svd_cv_dense_ex", "rcppml_gpu_svd_krylov_ex", "rcppml_gpu_svd_krylov_dense_ex",
    "rcppml_gpu_svd_reg_ex", "rcppml_gpu_svd_reg_dense_ex", "rcppml_gpu_svd_randomized_ex", "rcppml_gpu_svd_randomized_dense_ex",
    "rcppml_gpu_nmf_svd_init_ex", "rcppml_gpu_nmf_svd_init_dense_ex", "rcppml_hip_nmf_start_time",
    "rcppml_gpu_assess", "rcppml_gpu_assess_ex", "rcppml_gpu_knn_float", "rcppml_gpu_assess_plan",
    "rcppml_gpu_score_test_double", "rcppml_gpu_zero_inflation_double", "rcppml_gpu_dispersion_double",
    "rcppml_gpu_consensus_double", "rcppml_gpu_hclust_average_double",
    "rcppml_gpu_compute_target_double", "rcppml_gpu_refine_correct_double", "rcppml_gpu_refine_wfit_double", "rcppml_gpu_refine_double",
    "rcppml_gpu_nmf_zi_double", "rcppml_gpu_zi_em_double",
    "rcppml_gpu_classify_metrics_ex", "rcppml_gpu_classify_knn_ex", "rcppml_gpu_classify_logistic_ex",
    "rcppml_hip_graph_assemble", "rcppml_hip_graph_layer_loss", "rcppml_gpu_factor_net_fit_ex",
    "rcppml_gpu_cosine_sparse_ex", "rcppml_gpu_cosine_geometry", "rcppml_gpu_cosine_dense_ex", "rcppml_gpu_bipartite_match_ex",
]


class BackendError(RuntimeError):
    pass


class RhsPlan:
    """Owner of a rcppml_rhs_plan handle (device memory: free it with close() or let the GC do it)."""

    def __init__(self, handle):
        self._h = handle

    def info(self):
        out = (C.c_double * 11)()
        lib().rcppml_hip_rhs_plan_info(self._h, out)
        keys = ("partitions", "waves", "rounds", "slots", "workgroups_per_partition", "tiles", "slot_count", "spilled_nnz",
                "fill", "stream_bytes", "tiled_columns")
        d = {k: (float(out[i]) if k == "fill" else int(out[i])) for i, k in enumerate(keys)}
        d["kind"] = {1: "window", 0: "slab"}.get(int(lib().rcppml_hip_rhs_plan_kind(self._h)), "?")
        d["slot_rate"] = float(out[3])        # window plans: slots per column and phase (fractional); slab plans: S
        return d

    def close(self):
        if self._h is not None and self._h.value:
            lib().rcppml_hip_rhs_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lib():
    """Load RcppML_gpu.so (RTLD_GLOBAL, as R's dyn.load(local=FALSE) does: reference R/gpu_backend.R:87)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BackendError(
                "HIP backend missing: %s not built (run `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C rcppml_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        try:
            _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        except OSError as e:  # e.g. libamdhip64 missing
            raise BackendError("cannot load %s: %s" % (LIB_PATH, e))
        _lib.rcppml_gpu_last_error.restype = C.c_char_p
        for name in ("rcppml_hip_ctx_create", "rcppml_hip_ctx_sync", "rcppml_hip_ctx_stats", "rcppml_hip_ctx_set_option", "rcppml_hip_transpose_csc", "rcppml_hip_cast", "rcppml_hip_gram", "rcppml_hip_rhs",
                     "rcppml_hip_solve_cd", "rcppml_hip_order_columns", "rcppml_hip_solve_chol", "rcppml_hip_row_norms",
                     "rcppml_hip_apply_scaling",
                     "rcppml_hip_sumsq", "rcppml_hip_loss_mse", "rcppml_hip_solve_masked", "rcppml_hip_loss_nonzeros", "rcppml_hip_loss_masked",
                     "rcppml_hip_solve_irls_nb", "rcppml_hip_nb_size_update", "rcppml_hip_nb_loss", "rcppml_hip_scale_order",
                     "rcppml_hip_gram_loss_mse", "rcppml_hip_tail_scale_gram", "rcppml_hip_tail_scale_gram_loss"):
            getattr(_lib, name).restype = C.c_int
        _lib.rcppml_hip_ctx_destroy.restype = None
        _lib.rcppml_hip_rhs_plan_destroy.restype = None
        _lib.rcppml_hip_rhs_plan_destroy.argtypes = [C.c_void_p]
        for name in ("rcppml_hip_rhs_plan_create", "rcppml_hip_rhs_plan_create_indices", "rcppml_hip_rhs_plan_set_values",
                     "rcppml_hip_rhs_plan_info", "rcppml_hip_rhs_planned"):
            getattr(_lib, name).restype = C.c_int
        _lib.rcppml_hip_rhs_plan_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    return _lib


def small_eligible(m, n, nnz, k):
    """True when the one-kernel fit (rcppml_hip_als_small_fit) takes a plain sparse MSE fit of this size."""
    f = lib().rcppml_hip_als_small_eligible
    f.restype = C.c_int
    return bool(f(C.c_int(m), C.c_int(n), C.c_int64(nnz), C.c_int(k)))


def last_error():
    return lib().rcppml_gpu_last_error().decode("utf-8", "replace")


def _chk(rc, what):
    if rc != 0:
        raise BackendError("%s failed: %s" % (what, last_error()))


# ----------------------------------------------------------------------------- plugin boundary
def _check(r, what):
    """The result dict of an entry wrapper, or BackendError with the entry's reason."""
    if r["status"] != 0:
        raise BackendError("GPU %s failed: %s" % (what, r["error"]))
    return r


def detect(max_gpus=8):
    """rcppml_gpu_detect -> list of (total_mb, free_mb); [] if no device (reference R/gpu_backend.R:101-106)."""
    n, st, mx = C.c_int(0), C.c_int(0), C.c_int(max_gpus)
    tot = (C.c_double * max_gpus)()
    fre = (C.c_double * max_gpus)()
    lib().rcppml_gpu_detect(C.byref(n), tot, fre, C.byref(mx), C.byref(st))
    if st.value != 0:
        return []
    return [(tot[i], fre[i]) for i in range(n.value)]


def _ci(v):
    return C.byref(C.c_int(int(v)))


def _cd(v):
    return C.byref(C.c_double(float(v)))


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def nmf_unified(p, i, x, m, n, k, W_T, H, *, entry="float", max_iter=100, tol=1e-4, L1_H=0.0, L1_W=0.0, L2_H=0.0,
                L2_W=0.0, L21_H=0.0, L21_W=0.0, ortho_H=0.0, ortho_W=0.0, ub_H=0.0, ub_W=0.0, cd_maxit=100, verbose=0,
                seed=0, loss_every=1, patience=5, nonneg_W=1, nonneg_H=1, loss_type=0, huber_delta=1.0, irls_max_iter=5,
                irls_tol=1e-4, norm_type=0, projective=0, symmetric=0, solver_mode=0, gp_dispersion_mode=2,
                nb_size=(10.0, 1e6, 0.01), mask=None, cd_tol=1e-8, sort_model=1, precision=F64, want_history=False,
                graph_W_nnz=0, guide_H_count=0, tweedie_power=1.5, robust_delta=0.0, graph_W=None, graph_H=None,
                gp_theta=(0.1, 5.0, 0.0), gamma_phi=(1.0, 1e4, 1e-6), target_H=None, target_W=None, theta_capacity=None):
    """Call the 73-pointer plugin entry exactly as reference gpu/bridge_nmf.hpp:310-342 does.

    p, i: int32 CSC arrays; x: float64 values.  W_T (m, k) and H (n, k) float64 arrays (memory = column-major
    k x m / k x n) are updated IN PLACE.  entry: "float" | "double" (the reference symbols) or "ex" (build-defined,
    adds mask / cd_tol / sort / precision / loss history).  target_H / target_W = (matrix (n, k) / (m, k), lambda): target
    regularisation through the build-defined rcppml_gpu_nmf_target (entry "ex" arguments + targets).
    Returns dict(d, iter, converged, loss, tol, status, ...).
    """
    L = lib()
    p = np.ascontiguousarray(p, np.int32)
    i = np.ascontiguousarray(i, np.int32)
    x = np.ascontiguousarray(x, np.float64)
    assert W_T.dtype == np.float64 and H.dtype == np.float64 and W_T.flags.c_contiguous and H.flags.c_contiguous
    assert W_T.shape == (m, k) and H.shape == (n, k)
    d = np.ones(k, np.float64)
    dummy_i = np.zeros(2, np.int32)
    dummy_d = np.zeros(2, np.float64)
    # out_theta: m doubles in the reference bridge (gpu/bridge_nmf.hpp:284); the build-defined "ex" entries take max(m, n) so that
    # dispersion = "per_col" (gp_dispersion_mode 3) can return its n values
    # (theta_capacity: what the caller's buffer holds -- tests hand the "ex" entry the bridge's m doubles)
    theta = np.zeros(max(m, n, 1) if entry == "ex" else max(m, 1), np.float64)
    if theta_capacity is not None:
        theta = np.zeros(max(int(theta_capacity), 1), np.float64)
    # (the build-defined entries read *out_theta_len on input as the capacity of out_theta)
    out_iter, out_conv, out_status, out_theta_len = C.c_int(0), C.c_int(0), C.c_int(-99), C.c_int((theta.shape[0] if theta_capacity is None else int(theta_capacity)) if entry == "ex" else 0)
    out_loss, out_tol = C.c_double(0), C.c_double(0)
    args = [
        _np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k),
        _np_ptr(W_T), _np_ptr(H), _np_ptr(d), _ci(max_iter), _cd(tol),
        _cd(L1_H), _cd(L1_W), _cd(L2_H), _cd(L2_W), _cd(L21_H), _cd(L21_W), _cd(ortho_H), _cd(ortho_W),
        _cd(ub_H), _cd(ub_W), _ci(cd_maxit), _ci(verbose), _ci(seed), _ci(loss_every), _ci(patience),
        _ci(nonneg_W), _ci(nonneg_H), _ci(loss_type), _cd(huber_delta), _ci(irls_max_iter), _cd(irls_tol),
        _ci(norm_type), _ci(projective), _ci(symmetric), _ci(solver_mode),
        _np_ptr(dummy_i), _np_ptr(dummy_i), _np_ptr(dummy_d), _ci(0), _ci(graph_W_nnz), _cd(0.0),
        _np_ptr(dummy_i), _np_ptr(dummy_i), _np_ptr(dummy_d), _ci(0), _ci(0), _cd(0.0),
        _ci(gp_dispersion_mode), _cd(gp_theta[0]), _cd(gp_theta[1]), _cd(gp_theta[2]), _cd(nb_size[0]), _cd(nb_size[1]), _cd(nb_size[2]),
        _cd(gamma_phi[0]), _cd(gamma_phi[1]), _cd(gamma_phi[2]), _cd(robust_delta), _cd(tweedie_power),
        _np_ptr(theta), C.byref(out_theta_len),
        _np_ptr(dummy_i), _np_ptr(dummy_i), _np_ptr(dummy_d), _np_ptr(dummy_i), _ci(guide_H_count),
        C.byref(out_iter), C.byref(out_conv), C.byref(out_loss), C.byref(out_status), C.byref(out_tol),
    ]
    # graph_W / graph_H: (p, i, x, lambda) CSC Laplacians (m x m / n x n), reference bridge_nmf.hpp graph_* slots
    for slot, g, dim in ((37, graph_W, m), (43, graph_H, n)):
        if g is not None:
            gp, gi, gx, lam = g
            gp = np.ascontiguousarray(gp, np.int32); gi = np.ascontiguousarray(gi, np.int32); gx = np.ascontiguousarray(gx, np.float64)
            args[slot:slot + 6] = [_np_ptr(gp), _np_ptr(gi), _np_ptr(gx), _ci(gp.shape[0] - 1), _ci(gx.shape[0]), _cd(lam)]
            args.append((gp, gi, gx))          # keep alive; popped below
    keep = args[73:]
    del args[73:]
    assert len(args) == 73
    hist = None
    if entry == "float":
        L.rcppml_gpu_nmf_unified_float(*args)
    elif entry == "double":
        L.rcppml_gpu_nmf_unified_double(*args)
    elif entry == "ex":
        if mask is not None:
            mp = np.ascontiguousarray(mask[0], np.int32)
            mi = np.ascontiguousarray(mask[1], np.int32)
            mnnz = int(mi.shape[0])
        else:
            mp, mi, mnnz = dummy_i, dummy_i, 0
        hist = np.full(max(max_iter, 1), np.nan) if want_history else None
        if target_H is not None or target_W is not None:
            tH = np.ascontiguousarray(target_H[0], np.float64) if target_H is not None else None
            tW = np.ascontiguousarray(target_W[0], np.float64) if target_W is not None else None
            assert tH is None or tH.shape == (n, k)
            assert tW is None or tW.shape == (m, k)
            L.rcppml_gpu_nmf_target(*args, _np_ptr(mp), _np_ptr(mi), _ci(mnnz), _cd(cd_tol), _ci(sort_model), _ci(precision),
                                    _np_ptr(hist) if hist is not None else None,
                                    _np_ptr(tH) if tH is not None else None, _cd(target_H[1] if target_H is not None else 0.0),
                                    _np_ptr(tW) if tW is not None else None, _cd(target_W[1] if target_W is not None else 0.0))
        else:
            L.rcppml_gpu_nmf_ex(*args, _np_ptr(mp), _np_ptr(mi), _ci(mnnz), _cd(cd_tol), _ci(sort_model), _ci(precision),
                                _np_ptr(hist) if hist is not None else None)
    else:
        raise ValueError(entry)
    res = dict(d=d, iter=out_iter.value, converged=bool(out_conv.value), loss=out_loss.value, tol=out_tol.value,
               status=out_status.value, theta=theta[:out_theta_len.value].copy())
    if hist is not None:
        res["loss_history"] = hist[:out_iter.value].copy()
    if out_status.value != 0:
        res["error"] = last_error()
    return res


def nnls_double(p, i, x, m, n, k, w_T, h, *, cd_maxit=100, cd_tol=1e-8, L1=0.0, L2=0.0, ub=0.0, nonneg=1, warm=0):
    st = C.c_int(-99)
    p = np.ascontiguousarray(p, np.int32); i = np.ascontiguousarray(i, np.int32); x = np.ascontiguousarray(x, np.float64)
    assert w_T.shape == (m, k) and h.shape == (n, k) and w_T.dtype == np.float64 and h.dtype == np.float64
    lib().rcppml_gpu_nnls_double(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k),
                                 _np_ptr(np.ascontiguousarray(w_T)), _np_ptr(h), _ci(cd_maxit), _cd(cd_tol), _cd(L1),
                                 _cd(L2), _cd(ub), _ci(nonneg), _ci(warm), C.byref(st))
    if st.value != 0:
        raise BackendError("rcppml_gpu_nnls_double: " + last_error())
    return h


def evaluate_mse_double(p, i, x, m, n, k, W_T, d, H, mask_zeros=False):
    st, out = C.c_int(-99), C.c_double(0)
    p = np.ascontiguousarray(p, np.int32); i = np.ascontiguousarray(i, np.int32); x = np.ascontiguousarray(x, np.float64)
    lib().rcppml_gpu_evaluate_mse_double(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k),
                                         _np_ptr(np.ascontiguousarray(W_T, np.float64)),
                                         _np_ptr(np.ascontiguousarray(d, np.float64)),
                                         _np_ptr(np.ascontiguousarray(H, np.float64)), _ci(int(mask_zeros)),
                                         C.byref(out), C.byref(st))
    if st.value != 0:
        raise BackendError("rcppml_gpu_evaluate_mse_double: " + last_error())
    return out.value


PROFILE_PHASES = ("gram_H", "rhs_H", "nnls_H", "norm_H", "gram_W", "rhs_W_gather", "rhs_W_planned", "nnls_W", "norm_W", "loss", "total")


def nmf_profile_double(p, i, x, m, n, k, max_iter=10, tol=0.0, cd_maxit=10, seed=42):
    """rcppml_gpu_nmf_profile_double (reference src/gpu_bridge_utils.cu:48): per-phase HIP-event times of the batch-CD ALS
    iteration.  Returns dict(total_ms, per_iter_ms: {phase: ms}, iters)."""
    p = np.ascontiguousarray(p, np.int32); i = np.ascontiguousarray(i, np.int32); x = np.ascontiguousarray(x, np.float64)
    tot, per = np.zeros(11), np.zeros(11)
    it, st = C.c_int(0), C.c_int(-99)
    lib().rcppml_gpu_nmf_profile_double(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k), _ci(max_iter),
                                        _cd(tol), _ci(cd_maxit), _ci(seed), _np_ptr(tot), _np_ptr(per), C.byref(it), C.byref(st))
    if st.value != 0:
        raise BackendError("rcppml_gpu_nmf_profile_double: " + last_error())
    return dict(total_ms=dict(zip(PROFILE_PHASES, tot.tolist())), per_iter_ms=dict(zip(PROFILE_PHASES, per.tolist())), iters=it.value)


# ----------------------------------------------------------------------------- device-level ops
def _dptr(t):
    """Device pointer of a torch tensor (or raw int / None)."""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def nmf_cv(p, i, x, m, n, k, W_T, H, *, entry="ex", max_iter=100, tol=1e-4, L1_H=0.0, L1_W=0.0, L2_H=0.0, L2_W=0.0, cd_maxit=100,
           verbose=0, seed=0, holdout_fraction=0.1, cv_seed=0, mask_zeros=0, nonneg_W=1, nonneg_H=1, norm_type=0, loss_type=0,
           solver_mode=0, projective=0, symmetric=0, graph_W_nnz=0, sort_model=1, precision=F64, cv_patience=5,
           graph_W=None, graph_H=None, irls_max_iter=5, irls_tol=1e-4, dispersion_mode=2, gp_theta=(0.1, 5.0), tweedie_power=1.5,
           robust_delta=0.0, mask=None):
    """Call the CV plugin entry as reference gpu/bridge_nmf.hpp:407-497 does (51 pointers; entry "float" | "double"), or
    the build-defined "ex" form (+ sort flag, precision, patience, loss histories) or "irls_ex" (+ dispersion mode, GP theta
    init / max, Tweedie power, robust_delta; returns theta), or -- mask = (mask_p, mask_i) given -- "masked_ex" (irls_ex + the user mask).  W_T (m, k) and H (n, k) float64 arrays are updated IN PLACE (H
    returns with d absorbed).  loss_type 4..8: the IRLS CV path."""
    L = lib()
    p = np.ascontiguousarray(p, np.int32)
    i = np.ascontiguousarray(i, np.int32)
    x = np.ascontiguousarray(x, np.float64)
    assert W_T.dtype == np.float64 and H.dtype == np.float64 and W_T.flags.c_contiguous and H.flags.c_contiguous
    assert W_T.shape == (m, k) and H.shape == (n, k)
    d = np.ones(k, np.float64)
    dummy_i = np.zeros(2, np.int32)
    dummy_d = np.zeros(2, np.float64)
    out_iter, out_conv, out_best_iter, out_status = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(-99)
    out_train, out_test, out_best = C.c_double(0), C.c_double(0), C.c_double(0)
    args = [
        _np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k),
        _np_ptr(W_T), _np_ptr(H), _np_ptr(d), _ci(max_iter), _cd(tol),
        _cd(L1_H), _cd(L1_W), _cd(L2_H), _cd(L2_W), _ci(cd_maxit), _ci(verbose), _ci(seed),
        _cd(holdout_fraction), _ci(cv_seed), _ci(mask_zeros), _ci(nonneg_W), _ci(nonneg_H), _ci(norm_type),
        _ci(loss_type), _cd(1.0), _ci(irls_max_iter), _cd(irls_tol),
        _np_ptr(dummy_i), _np_ptr(dummy_i), _np_ptr(dummy_d), _ci(0), _ci(graph_W_nnz), _cd(0.0),
        _np_ptr(dummy_i), _np_ptr(dummy_i), _np_ptr(dummy_d), _ci(0), _ci(0), _cd(0.0),
        _ci(projective), _ci(symmetric), _ci(solver_mode),
        C.byref(out_iter), C.byref(out_conv), C.byref(out_train), C.byref(out_test), C.byref(out_best), C.byref(out_best_iter),
        C.byref(out_status),
    ]
    keep = []
    for slot, g in ((29, graph_W), (35, graph_H)):          # (p, i, x, lambda) CSC Laplacians, as in nmf_unified
        if g is not None:
            gp, gi, gx, lam = g
            gp = np.ascontiguousarray(gp, np.int32); gi = np.ascontiguousarray(gi, np.int32); gx = np.ascontiguousarray(gx, np.float64)
            args[slot:slot + 6] = [_np_ptr(gp), _np_ptr(gi), _np_ptr(gx), _ci(gp.shape[0] - 1), _ci(gx.shape[0]), _cd(lam)]
            keep.append((gp, gi, gx))
    assert len(args) == 51
    th = eh = None
    theta = None
    if mask is not None:
        mp = np.ascontiguousarray(mask[0], np.int32); mi = np.ascontiguousarray(mask[1], np.int32)
        if mi.shape[0] == 0:
            mi = np.zeros(1, np.int32)
        th = np.full(max(max_iter, 1), np.nan)
        eh = np.full(max(max_iter, 1), np.nan)
        theta = np.zeros(max(m, 1), np.float64)
        fn = L.rcppml_gpu_nmf_cv_masked_ex
        fn.restype = None
        fn(*args, _ci(sort_model), _ci(precision), _ci(cv_patience), _np_ptr(th), _np_ptr(eh), _ci(dispersion_mode), _cd(gp_theta[0]),
           _cd(gp_theta[1]), _cd(tweedie_power), _cd(robust_delta), _np_ptr(theta), _np_ptr(mp), _np_ptr(mi), _ci(int(mp[-1])))
    elif entry == "irls_ex":
        th = np.full(max(max_iter, 1), np.nan)
        eh = np.full(max(max_iter, 1), np.nan)
        theta = np.zeros(max(m, 1), np.float64)
        fn = L.rcppml_gpu_nmf_cv_irls_ex
        fn.restype = None
        fn(*args, _ci(sort_model), _ci(precision), _ci(cv_patience), _np_ptr(th), _np_ptr(eh), _ci(dispersion_mode), _cd(gp_theta[0]),
           _cd(gp_theta[1]), _cd(tweedie_power), _cd(robust_delta), _np_ptr(theta))
    elif entry == "ex":
        th = np.full(max(max_iter, 1), np.nan)
        eh = np.full(max(max_iter, 1), np.nan)
        fn = L.rcppml_gpu_nmf_cv_ex
        fn.restype = None
        fn(*args, _ci(sort_model), _ci(precision), _ci(cv_patience), _np_ptr(th), _np_ptr(eh))
    else:
        fn = getattr(L, "rcppml_gpu_nmf_cv_unified_" + entry)
        fn.restype = None
        fn(*args)
    res = dict(status=out_status.value, iter=out_iter.value, converged=bool(out_conv.value), train_loss=out_train.value,
               test_loss=out_test.value, best_test_loss=out_best.value, best_iter=out_best_iter.value, d=d)
    if out_status.value != 0:
        res["error"] = last_error()
    if th is not None:
        res["train_history"], res["test_history"] = th[:out_iter.value].copy(), eh[:out_iter.value].copy()
    if theta is not None:
        res["theta"] = theta
    return res


def nmf_zerocopy(d_col_ptr, d_row_idx, d_values, m, n, nnz, k, W_T, H, *, max_iter=100, tol=1e-4, L1_H=0.0, L1_W=0.0, L2_H=0.0,
                 L2_W=0.0, L21_H=0.0, L21_W=0.0, ortho_H=0.0, ortho_W=0.0, ub_H=0.0, ub_W=0.0, cd_maxit=100, verbose=0, seed=0,
                 patience=5, nonneg_W=1, nonneg_H=1, loss_type=0, norm_type=0):
    """Call rcppml_gpu_nmf_zerocopy_double as R/sp_gpu.R does: d_col_ptr / d_row_idx (int32) and d_values (float64) are
    DEVICE tensors (torch) or raw device addresses; addresses travel as doubles."""
    L = lib()

    def addr(t):
        return float(t.data_ptr()) if hasattr(t, "data_ptr") else float(t)

    d = np.ones(k, np.float64)
    out_iter, out_conv, out_status = C.c_int(0), C.c_int(0), C.c_int(-99)
    out_loss, out_tol = C.c_double(0), C.c_double(0)
    fn = L.rcppml_gpu_nmf_zerocopy_double
    fn.restype = None
    fn(_cd(addr(d_col_ptr)), _cd(addr(d_row_idx)), _cd(addr(d_values)), _ci(m), _ci(n), _cd(float(nnz)), _ci(k),
       _np_ptr(W_T), _np_ptr(H), _np_ptr(d), _ci(max_iter), _cd(tol), _cd(L1_H), _cd(L1_W), _cd(L2_H), _cd(L2_W), _cd(L21_H),
       _cd(L21_W), _cd(ortho_H), _cd(ortho_W), _cd(ub_H), _cd(ub_W), _ci(cd_maxit), _ci(verbose), _ci(seed), _ci(1),
       _ci(patience), _ci(nonneg_W), _ci(nonneg_H), _ci(loss_type), _cd(1.0), _ci(5), _cd(1e-4), _ci(norm_type),
       C.byref(out_iter), C.byref(out_conv), C.byref(out_loss), C.byref(out_status), C.byref(out_tol))
    res = dict(status=out_status.value, iter=out_iter.value, converged=bool(out_conv.value), loss=out_loss.value, tol=out_tol.value, d=d)
    if out_status.value != 0:
        res["error"] = last_error()
    return res


class Context:
    """rcppml_hip_ctx bound to a device and a HIP stream (default: torch's current stream on that device)."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(device).cuda_stream
        _chk(lib().rcppml_hip_ctx_create(C.byref(self._h), C.c_int(device), C.c_void_p(stream)), "ctx_create")
        self.device = device

    def close(self):
        if self._h:
            lib().rcppml_hip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _chk(lib().rcppml_hip_ctx_sync(self._h), "ctx_sync")

    def set_option(self, option, value):
        if option == OPT_CD_PRIO and not cd_prio_valid(value):
            raise BackendError("ctx_set_option: RCPPML_OPT_CD_PRIO value %r is out of range" % (value,))
        _chk(lib().rcppml_hip_ctx_set_option(self._h, C.c_int(option), C.c_int(value)), "ctx_set_option")

    def stats(self, reset=False):
        """Work counters since creation / the last reset (synchronises): cd_column_sweeps, cd_columns; cd_slot_sweeps (persistent
        LMF kernel: column slots x wave sweeps, idle and correction sweeps included) and cd_noop_steps (OPT_CD_COUNT_NOOP)."""
        out = (C.c_ulonglong * 4)()
        _chk(lib().rcppml_hip_ctx_stats(self._h, C.c_int(1 if reset else 0), out), "ctx_stats")
        return dict(cd_column_sweeps=int(out[0]), cd_columns=int(out[1]), cd_slot_sweeps=int(out[2]), cd_noop_steps=int(out[3]))

    def cd_step_stats(self, reset=False):
        """Per-(column, coordinate) steps of the lane = column CD kernel (only counted while OPT_CD_COUNT_NOOP is set): steps whose
        update is exactly 0 (the reference skips them) and all steps of live columns."""
        out = (C.c_ulonglong * 2)()
        _chk(lib().rcppml_hip_ctx_cd_step_stats(self._h, C.c_int(1 if reset else 0), out), "ctx_cd_step_stats")
        return dict(cd_zero_steps=int(out[0]), cd_steps=int(out[1]))

    def irls_stats(self, reset=False):
        """IRLS work counters (only counted while OPT_CD_COUNT_NOOP is set): passes over columns, nonzero-passes."""
        out = (C.c_ulonglong * 2)()
        _chk(lib().rcppml_hip_ctx_irls_stats(self._h, C.c_int(1 if reset else 0), out), "ctx_irls_stats")
        sw = (C.c_ulonglong * 1)()
        _chk(lib().rcppml_hip_ctx_irls_sweep_stats(self._h, C.c_int(1 if reset else 0), sw), "ctx_irls_sweep_stats")
        return dict(irls_column_passes=int(out[0]), irls_nonzero_passes=int(out[1]), irls_cd_sweeps=int(sw[0]))

    def transpose_csc(self, dt, rows, cols, col_ptr, row_idx, values, t_col_ptr, t_row_idx, t_values):
        _chk(lib().rcppml_hip_transpose_csc(self._h, C.c_int(dt), C.c_int(rows), C.c_int(cols), _dptr(col_ptr), _dptr(row_idx),
                                            _dptr(values), _dptr(t_col_ptr), _dptr(t_row_idx), _dptr(t_values)), "transpose_csc")

    def cast(self, dt_src, src, dt_dst, dst, n):
        _chk(lib().rcppml_hip_cast(self._h, C.c_int(dt_src), _dptr(src), C.c_int(dt_dst), _dptr(dst), C.c_int64(n)), "cast")

    # ---- ops (dt: F32/F64; tensors are torch CUDA tensors laid out (cols, k) == column-major k x cols)
    def gram(self, dt, F, k, r, eps, l2, G):
        _chk(lib().rcppml_hip_gram(self._h, C.c_int(dt), _dptr(F), C.c_int(k), C.c_int64(r), C.c_double(eps),
                                   C.c_double(l2), _dptr(G)), "gram")

    def rhs(self, dt, col_ptr, row_idx, values, ncols, F, k, B):
        _chk(lib().rcppml_hip_rhs(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values), C.c_int64(ncols),
                                  _dptr(F), C.c_int(k), _dptr(B)), "rhs")

    def rhs_plan(self, dt, col_ptr, row_idx, values, ncols, nrows, k, partitions=0, slots=0):
        """Tile-partitioned slot copy of one CSC matrix for the LDS row-tiled kernel; None when the shape is not eligible
        (the caller then keeps using rhs())."""
        h = C.c_void_p()
        _chk(lib().rcppml_hip_rhs_plan_create(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values), C.c_int64(ncols),
                                              C.c_int64(nrows), C.c_int(k), C.c_int(partitions), C.c_int(slots), C.byref(h)), "rhs_plan_create")
        return RhsPlan(h) if h.value else None

    def rhs_plan_indices(self, dt, col_ptr, row_idx, ncols, nrows, k, partitions=0, slots=0):
        """The index half of a window plan (no values yet); None when the window planner declines.  Then rhs_plan_set_values."""
        h = C.c_void_p()
        _chk(lib().rcppml_hip_rhs_plan_create_indices(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), C.c_int64(ncols),
                                                      C.c_int64(nrows), C.c_int(k), C.c_int(partitions), C.c_int(slots), C.byref(h)),
             "rhs_plan_create_indices")
        return RhsPlan(h) if h.value else None

    def rhs_plan_set_values(self, plan, values):
        _chk(lib().rcppml_hip_rhs_plan_set_values(self._h, plan._h, _dptr(values)), "rhs_plan_set_values")

    def rhs_planned(self, plan, F, B):
        _chk(lib().rcppml_hip_rhs_planned(self._h, plan._h, _dptr(F), _dptr(B)), "rhs_planned")

    def solve_cd(self, dt, G, B, X, k, ncols, l1_pre=0.0, warm=0, zero_init=0, l1_cd=0.0, l2_cd=0.0, nonneg=1, maxit=100,
                 tol=1e-8, ub_cd=0.0, ub_post=0.0, variant=CD_AUTO, sweeps_out=None, col_order=None):
        _chk(lib().rcppml_hip_solve_cd(self._h, C.c_int(dt), _dptr(G), _dptr(B), _dptr(X), C.c_int(k), C.c_int64(ncols),
                                       C.c_double(l1_pre), C.c_int(warm), C.c_int(zero_init), C.c_double(l1_cd),
                                       C.c_double(l2_cd), C.c_int(nonneg), C.c_int(maxit), C.c_double(tol),
                                       C.c_double(ub_cd), C.c_double(ub_post), C.c_int(variant), _dptr(sweeps_out), _dptr(col_order)), "solve_cd")

    def order_columns(self, sweeps, ncols, order):
        _chk(lib().rcppml_hip_order_columns(self._h, _dptr(sweeps), C.c_int64(ncols), _dptr(order)), "order_columns")

    def solve_chol(self, dt, G, B, X, k, ncols, l1_pre=0.0, nonneg=1, ub_post=0.0):
        _chk(lib().rcppml_hip_solve_chol(self._h, C.c_int(dt), _dptr(G), _dptr(B), _dptr(X), C.c_int(k), C.c_int64(ncols),
                                         C.c_double(l1_pre), C.c_int(nonneg), C.c_double(ub_post)), "solve_chol")

    def row_norms(self, dt, X, k, ncols, norm_type, out):
        _chk(lib().rcppml_hip_row_norms(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols), C.c_int(norm_type),
                                        _dptr(out)), "row_norms")

    def apply_scaling(self, dt, X, k, ncols, norm_type, sums, d):
        _chk(lib().rcppml_hip_apply_scaling(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols),
                                            C.c_int(norm_type), _dptr(sums), _dptr(d)), "apply_scaling")

    def scale_order(self, dt, X, k, ncols, norm_type, sums, d, sweeps=None, order=None):
        """row_norms + apply_scaling (+ order_columns for the next solve) in three launches instead of five; bit-identical to the separate calls."""
        _chk(lib().rcppml_hip_scale_order(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols), C.c_int(norm_type),
                                          _dptr(sums), _dptr(d), _dptr(sweeps), _dptr(order)), "scale_order")

    def gram_loss_mse(self, dt, W_T, k, m, eps, trAtA, d, B_w, G_saved, G_wt, out):
        """gram(W_T, eps) -> G_wt, then loss_mse with it, in three launches instead of four; bit-identical to the separate calls."""
        _chk(lib().rcppml_hip_gram_loss_mse(self._h, C.c_int(dt), _dptr(W_T), C.c_int(k), C.c_int64(m), C.c_double(eps), _dptr(trAtA),
                                            _dptr(d), _dptr(B_w), _dptr(G_saved), _dptr(G_wt), _dptr(out)), "gram_loss_mse")

    def tail_scale_gram(self, dt, X, k, ncols, norm_type, sums, d, sweeps, order, eps, l2, G):
        """scale_order(X) then gram(X, eps, l2) -> G in one call (fp32 k = 64: the scaling inside the Gram's partial-tile kernel)."""
        _chk(lib().rcppml_hip_tail_scale_gram(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols), C.c_int(norm_type), _dptr(sums),
                                              _dptr(d), _dptr(sweeps), _dptr(order), C.c_double(eps), C.c_double(l2), _dptr(G)), "tail_scale_gram")

    def tail_scale_gram_loss(self, dt, W_T, k, m, norm_type, sums, d, sweeps, order, eps, trAtA, B_w, G_saved, G_wt, out):
        """scale_order(W_T) then gram_loss_mse in one call (fp32 k = 64: the scaling inside the Gram's partial-tile kernel)."""
        _chk(lib().rcppml_hip_tail_scale_gram_loss(self._h, C.c_int(dt), _dptr(W_T), C.c_int(k), C.c_int64(m), C.c_int(norm_type), _dptr(sums),
                                                   _dptr(d), _dptr(sweeps), _dptr(order), C.c_double(eps), _dptr(trAtA), _dptr(B_w),
                                                   _dptr(G_saved), _dptr(G_wt), _dptr(out)), "tail_scale_gram_loss")

    def graph_assemble(self, mode, H, k, n, Z, p, X, dt=F64):
        """X (n x c, column-major) from the branch factors H (a list of (n, k_b) tensors = column-major k_b x n) and the condition block
        Z ((n, p) tensor or None); mode 0 concat, 1 add.  One launch, exact (rcppml_hip_graph_assemble)."""
        ptrs = (C.c_void_p * len(H))(*[h.data_ptr() for h in H])
        ks = (C.c_int * len(k))(*[int(v) for v in k])
        _chk(lib().rcppml_hip_graph_assemble(self._h, C.c_int(dt), C.c_int(mode), C.c_int(len(H)), ptrs, ks, C.c_int64(n), _dptr(Z),
                                             C.c_int(p), _dptr(X)), "graph_assemble")

    def graph_layer_loss(self, X, rows, c, W_T, d, H, k, scale, out, dt=F64):
        """out[0] = scale * ||X - W diag(d) H||_F^2 for a dense X (rows x c, column-major); two launches, bitwise-repeatable
        (rcppml_hip_graph_layer_loss)."""
        _chk(lib().rcppml_hip_graph_layer_loss(self._h, C.c_int(dt), _dptr(X), C.c_int64(rows), C.c_int(c), _dptr(W_T), _dptr(d), _dptr(H),
                                               C.c_int(k), C.c_double(scale), _dptr(out)), "graph_layer_loss")

    def als_small_fit(self, dt, csc, csc_t, m, n, k, W, H, d, trAtA, *, L1_H=0.0, L1_W=0.0, L2_H=0.0, L2_W=0.0, ub_H=0.0, ub_W=0.0, nonneg_H=1,
                      nonneg_W=1, norm_type=0, solver_mode=0, cd_maxit=100, cd_tol=1e-8, max_iter=100, tol=1e-4, patience=5, iter0=0, loss_history=None,
                      result8=None):
        """The whole plain sparse MSE fit as one persistent kernel (small problems only: small_eligible)."""
        _chk(lib().rcppml_hip_als_small_fit(self._h, C.c_int(dt), _dptr(csc["p"]), _dptr(csc["i"]), _dptr(csc["x"]), _dptr(csc_t["p"]),
                                            _dptr(csc_t["i"]), _dptr(csc_t["x"]), C.c_int(m), C.c_int(n), C.c_int64(csc["nnz"]), C.c_int(k),
                                            _dptr(W), _dptr(H), _dptr(d), _dptr(trAtA), C.c_double(L1_H), C.c_double(L1_W), C.c_double(L2_H),
                                            C.c_double(L2_W), C.c_double(ub_H), C.c_double(ub_W), C.c_int(nonneg_H), C.c_int(nonneg_W),
                                            C.c_int(norm_type), C.c_int(solver_mode), C.c_int(cd_maxit), C.c_double(cd_tol), C.c_int(max_iter),
                                            C.c_double(tol), C.c_int(patience), C.c_int(iter0), _dptr(loss_history), _dptr(result8)), "als_small_fit")

    def sumsq(self, dt, x, length, out):
        _chk(lib().rcppml_hip_sumsq(self._h, C.c_int(dt), _dptr(x), C.c_int64(length), _dptr(out)), "sumsq")

    def loss_mse(self, dt, trAtA, d, W_T, B_w, k, m, G_wt, G_saved, out):
        _chk(lib().rcppml_hip_loss_mse(self._h, C.c_int(dt), _dptr(trAtA), _dptr(d), _dptr(W_T), _dptr(B_w), C.c_int(k),
                                       C.c_int64(m), _dptr(G_wt), _dptr(G_saved), _dptr(out)), "loss_mse")

    def solve_masked(self, dt, col_ptr, row_idx, values, mask_p, mask_i, ncols, F, G_full, X, k, l1=0.0, l2=0.0, nonneg=1,
                     cd_maxit=100, cd_tol=1e-8, solver_mode=0, warm=0):
        _chk(lib().rcppml_hip_solve_masked(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                           _dptr(mask_p), _dptr(mask_i), C.c_int64(ncols), _dptr(F), _dptr(G_full),
                                           _dptr(X), C.c_int(k), C.c_double(l1), C.c_double(l2), C.c_int(nonneg),
                                           C.c_int(cd_maxit), C.c_double(cd_tol), C.c_int(solver_mode), C.c_int(warm)),
             "solve_masked")

    def loss_masked(self, dt, loss_type, col_ptr, row_idx, values, mask_p, mask_i, ncols, W_T, d, H, k, out, power=1.5):
        _chk(lib().rcppml_hip_loss_masked(self._h, C.c_int(dt), C.c_int(loss_type), C.c_double(power), _dptr(col_ptr), _dptr(row_idx),
                                          _dptr(values), _dptr(mask_p), _dptr(mask_i), C.c_int64(ncols), _dptr(W_T), _dptr(d),
                                          _dptr(H), C.c_int(k), _dptr(out)), "loss_masked")

    def loss_nonzeros(self, dt, col_ptr, row_idx, values, mask_p, mask_i, ncols, W_T, d, H, k, out):
        _chk(lib().rcppml_hip_loss_nonzeros(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                            _dptr(mask_p), _dptr(mask_i), C.c_int64(ncols), _dptr(W_T), _dptr(d),
                                            _dptr(H), C.c_int(k), _dptr(out)), "loss_nonzeros")

    def solve_irls_nb(self, dt, col_ptr, row_idx, values, ncols, F, G_base, X, k, l1=0.0, l2=0.0, nonneg=1, cd_maxit=100,
                      irls_max_iter=5, irls_tol=1e-4, theta_row=None, theta_col=None):
        _chk(lib().rcppml_hip_solve_irls_nb(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                            C.c_int64(ncols), _dptr(F), _dptr(G_base), _dptr(X), C.c_int(k), C.c_double(l1),
                                            C.c_double(l2), C.c_int(nonneg), C.c_int(cd_maxit), C.c_int(irls_max_iter),
                                            C.c_double(irls_tol), _dptr(theta_row), _dptr(theta_col)), "solve_irls_nb")

    def solve_irls(self, dt, loss_type, col_ptr, row_idx, values, ncols, F, G_base, X, k, l1=0.0, l2=0.0, nonneg=1, cd_maxit=100,
                   irls_max_iter=5, irls_tol=1e-4, theta_row=None, theta_col=None, loss_param=0.0, robust_delta=0.0):
        _chk(lib().rcppml_hip_solve_irls(self._h, C.c_int(dt), C.c_int(loss_type), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                         C.c_int64(ncols), _dptr(F), _dptr(G_base), _dptr(X), C.c_int(k), C.c_double(l1),
                                         C.c_double(l2), C.c_int(nonneg), C.c_int(cd_maxit), C.c_int(irls_max_iter),
                                         C.c_double(irls_tol), _dptr(theta_row), _dptr(theta_col), C.c_double(loss_param),
                                         C.c_double(robust_delta)), "solve_irls")

    def irls_loss(self, dt, loss_type, col_ptr, row_idx, values, ncols, W_T, d, H, theta_row, k, out, loss_param=0.0, robust_delta=0.0):
        _chk(lib().rcppml_hip_irls_loss(self._h, C.c_int(dt), C.c_int(loss_type), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                        C.c_int64(ncols), _dptr(W_T), _dptr(d), _dptr(H), _dptr(theta_row), C.c_int(k),
                                        C.c_double(loss_param), C.c_double(robust_delta), _dptr(out)), "irls_loss")

    def solve_cv(self, dt, col_ptr, row_idx, values, ncols, nrows, F, G, X, k, frac, cv_seed, mask_zeros=0, transposed=0, l1=0.0,
                 nonneg=1, cd_maxit=100, solver_mode=0):
        _chk(lib().rcppml_hip_solve_cv(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values), C.c_int64(ncols),
                                       C.c_int(nrows), _dptr(F), _dptr(G), _dptr(X), C.c_int(k), C.c_double(frac),
                                       C.c_ulonglong(cv_seed), C.c_int(mask_zeros), C.c_int(transposed), C.c_double(l1),
                                       C.c_int(nonneg), C.c_int(cd_maxit), C.c_int(solver_mode)), "solve_cv")

    def set_cv_mask(self, mask_p=None, mask_i=None, maskT_p=None, maskT_i=None):
        """The user mask of a cross-validation fit: pattern CSC (int32 device arrays) of the mask and of its transpose, which must stay
        alive until the mask is cleared -- all four None.  While set, solve_cv, solve_cv_irls and cv_irls_loss honour it."""
        _chk(lib().rcppml_hip_ctx_set_cv_mask(self._h, _dptr(mask_p), _dptr(mask_i), _dptr(maskT_p), _dptr(maskT_i)), "ctx_set_cv_mask")

    def cv_test_error(self, dt, col_ptr, row_idx, values, ncols, nrows, W_T, d, H, k, frac, cv_seed, mask_zeros, out2):
        _chk(lib().rcppml_hip_cv_test_error(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values), C.c_int64(ncols),
                                            C.c_int(nrows), _dptr(W_T), _dptr(d), _dptr(H), C.c_int(k), C.c_double(frac),
                                            C.c_ulonglong(cv_seed), C.c_int(mask_zeros), _dptr(out2)), "cv_test_error")

    def solve_cv_irls(self, dt, loss_type, col_ptr, row_idx, values, ncols, nrows, F, G_add, X, k, frac, cv_seed, mask_zeros=0, transposed=0,
                      l1=0.0, nonneg=1, cd_maxit=100, solver_mode=0, irls_max_iter=5, irls_tol=1e-4, loss_param=1.5, robust_delta=0.0):
        _chk(lib().rcppml_hip_solve_cv_irls(self._h, C.c_int(dt), C.c_int(loss_type), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                            C.c_int64(ncols), C.c_int(nrows), _dptr(F), _dptr(G_add) if G_add is not None else None,
                                            _dptr(X), C.c_int(k), C.c_double(frac), C.c_ulonglong(cv_seed), C.c_int(mask_zeros),
                                            C.c_int(transposed), C.c_double(l1), C.c_int(nonneg), C.c_int(cd_maxit), C.c_int(solver_mode),
                                            C.c_int(irls_max_iter), C.c_double(irls_tol), C.c_double(loss_param), C.c_double(robust_delta)),
             "solve_cv_irls")

    def cv_irls_loss(self, dt, loss_type, col_ptr, row_idx, values, ncols, nrows, W_T, d, H, theta_row, k, frac, cv_seed, mask_zeros,
                     loss_param, out4):
        _chk(lib().rcppml_hip_cv_irls_loss(self._h, C.c_int(dt), C.c_int(loss_type), _dptr(col_ptr), _dptr(row_idx), _dptr(values),
                                           C.c_int64(ncols), C.c_int(nrows), _dptr(W_T), _dptr(d), _dptr(H),
                                           _dptr(theta_row) if theta_row is not None else None, C.c_int(k), C.c_double(frac),
                                           C.c_ulonglong(cv_seed), C.c_int(mask_zeros), C.c_double(loss_param), _dptr(out4)), "cv_irls_loss")

    def cv_gp_theta_update(self, dt, mode, t_col_ptr, t_row_idx, t_values, m, nnz, W_T, d, H, n, k, frac, cv_seed, theta_max, theta):
        _chk(lib().rcppml_hip_cv_gp_theta_update(self._h, C.c_int(dt), C.c_int(mode), _dptr(t_col_ptr), _dptr(t_row_idx), _dptr(t_values),
                                                 C.c_int64(m), C.c_int64(nnz), _dptr(W_T), _dptr(d), _dptr(H), C.c_int64(n), C.c_int(k),
                                                 C.c_double(frac), C.c_ulonglong(cv_seed), C.c_double(theta_max), _dptr(theta)),
             "cv_gp_theta_update")

    def apply_graph_reg(self, dt, G, lap_p, lap_i, lap_x, X, k, ncols, lam):
        _chk(lib().rcppml_hip_apply_graph_reg(self._h, C.c_int(dt), _dptr(G), _dptr(lap_p), _dptr(lap_i), _dptr(lap_x), _dptr(X),
                                              C.c_int(k), C.c_int64(ncols), C.c_double(lam)), "apply_graph_reg")

    def apply_l21(self, dt, G, X, k, ncols, lam):
        _chk(lib().rcppml_hip_apply_l21(self._h, C.c_int(dt), _dptr(G), _dptr(X), C.c_int(k), C.c_int64(ncols), C.c_double(lam)), "apply_l21")

    def angular_posthoc(self, dt, X, k, ncols, lam):
        _chk(lib().rcppml_hip_angular_posthoc(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols), C.c_double(lam)), "angular_posthoc")

    def dispersion_update(self, dt, loss_type, mode, t_col_ptr, t_row_idx, t_values, m, nnz, W_T, d, H, n, k, power, lo, hi, theta):
        _chk(lib().rcppml_hip_dispersion_update(self._h, C.c_int(dt), C.c_int(loss_type), C.c_int(mode), _dptr(t_col_ptr),
                                                _dptr(t_row_idx), _dptr(t_values), C.c_int64(m), C.c_int64(nnz), _dptr(W_T), _dptr(d),
                                                _dptr(H), C.c_int64(n), C.c_int(k), C.c_double(power), C.c_double(lo),
                                                C.c_double(hi), _dptr(theta)), "dispersion_update")

    def mul_rows(self, dt, X, k, ncols, d, Y):
        """Y = diag(d) X."""
        _chk(lib().rcppml_hip_mul_rows(self._h, C.c_int(dt), _dptr(X), C.c_int(k), C.c_int64(ncols), _dptr(d), _dptr(Y)), "mul_rows")

    def axpy(self, dt, X, T, alpha, n, Y):
        """Y = X + alpha T over n entries."""
        _chk(lib().rcppml_hip_axpy(self._h, C.c_int(dt), _dptr(X), _dptr(T), C.c_double(alpha), C.c_int64(n), _dptr(Y)), "axpy")

    def clip_upper(self, dt, X, n, ub):
        """X = min(X, ub) over n entries, in place."""
        _chk(lib().rcppml_hip_clip_upper(self._h, C.c_int(dt), _dptr(X), C.c_int64(n), C.c_double(ub)), "clip_upper")

    def vec_global(self, dt, stat, x, m):
        _chk(lib().rcppml_hip_vec_global(self._h, C.c_int(dt), C.c_int(stat), _dptr(x), C.c_int64(m)), "vec_global")

    def rhs_dense(self, dt, A, m, n, transposed, F, k, B):
        _chk(lib().rcppml_hip_rhs_dense(self._h, C.c_int(dt), _dptr(A), C.c_int64(m), C.c_int64(n), C.c_int(transposed), _dptr(F),
                                        C.c_int(k), _dptr(B)), "rhs_dense")

    @staticmethod
    def rhs_dense_geometry(dt, m, n, k, transposed):
        """The launch geometry rhs_dense uses for this problem (host arithmetic only): blocks of output columns, slices of the
        reduction (1 = B written directly, no reduce kernel), reduction indices per slice (a multiple of the 32- / 16-index chunk of
        the forward / backward kernels) and the kernels' row-tile template parameter."""
        out = (C.c_int64 * 4)()
        _chk(lib().rcppml_hip_rhs_dense_geometry(C.c_int(dt), C.c_int64(m), C.c_int64(n), C.c_int(k), C.c_int(transposed), out),
             "rhs_dense_geometry")
        return dict(zip(("blocks", "slices", "rows_per_slice", "row_tiles"), (int(v) for v in out)))

    def spz_decode(self, file_bytes, d_col_ptr, d_row_idx, d_values):
        """file_bytes: uint8 numpy array (host); outputs: device int32 (n+1), int32 (nnz), float64 (nnz)."""
        buf = np.ascontiguousarray(file_bytes, np.uint8)
        st = lib().rcppml_hip_spz_decode(self._h, buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size), _dptr(d_col_ptr),
                                         _dptr(d_row_idx), _dptr(d_values))
        if st != 0:
            raise BackendError("spz_decode failed (status %d): %s" % (st, last_error()))

    def nb_size_update(self, dt, t_col_ptr, t_row_idx, t_values, m, W_T, d, H, n, k, r_min, r_max, nb_size):
        _chk(lib().rcppml_hip_nb_size_update(self._h, C.c_int(dt), _dptr(t_col_ptr), _dptr(t_row_idx), _dptr(t_values),
                                             C.c_int64(m), _dptr(W_T), _dptr(d), _dptr(H), C.c_int64(n), C.c_int(k),
                                             C.c_double(r_min), C.c_double(r_max), _dptr(nb_size)), "nb_size_update")

    def nb_size_update_loss(self, dt, t_col_ptr, t_row_idx, t_values, m, nnz, W_T, d, H, n, k, r_min, r_max, nb_size, out):
        """nb_size_update followed by nb_loss with the updated sizes, in one pass over CSC(A^T) (per-row dispersion)."""
        _chk(lib().rcppml_hip_nb_size_update_loss(self._h, C.c_int(dt), _dptr(t_col_ptr), _dptr(t_row_idx), _dptr(t_values),
                                                  C.c_int64(m), C.c_int64(nnz), _dptr(W_T), _dptr(d), _dptr(H), C.c_int64(n),
                                                  C.c_int(k), C.c_double(r_min), C.c_double(r_max), _dptr(nb_size), _dptr(out)),
             "nb_size_update_loss")

    def nb_loss(self, dt, col_ptr, row_idx, values, ncols, W_T, d, H, theta_row, k, out):
        _chk(lib().rcppml_hip_nb_loss(self._h, C.c_int(dt), _dptr(col_ptr), _dptr(row_idx), _dptr(values), C.c_int64(ncols),
                                      _dptr(W_T), _dptr(d), _dptr(H), _dptr(theta_row), C.c_int(k), _dptr(out)), "nb_loss")


def spz_info(file_bytes):
    """Header of a .spz v2 byte stream: (status, m, n, nnz, value_type); host only."""
    buf = np.ascontiguousarray(file_bytes, np.uint8)
    m, n, vt, nnz = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
    st = lib().rcppml_hip_spz_info(buf.ctypes.data_as(C.c_void_p), C.c_uint64(buf.size), C.byref(m), C.byref(n), C.byref(nnz), C.byref(vt))
    return st, m.value, n.value, nnz.value, vt.value


def sp_read_gpu(path, device=0):
    """reference R/sp_gpu.R sp_read_gpu -> rcppml_sp_read_gpu: dict(status, m, n, nnz, col_ptr, row_idx, values) with the
    three device addresses as floats, exactly as the .C() call returns them."""
    pth = C.c_char_p(os.fsencode(path))
    dev = C.c_int(device)
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    m, n, st = C.c_int(0), C.c_int(0), C.c_int(-99)
    nnz = C.c_double(0)
    lib().rcppml_sp_read_gpu(C.byref(pth), C.byref(dev), C.byref(a), C.byref(b), C.byref(c), C.byref(m), C.byref(n), C.byref(nnz), C.byref(st))
    return dict(status=st.value, m=m.value, n=n.value, nnz=int(nnz.value), col_ptr=a.value, row_idx=b.value, values=c.value,
                error=last_error() if st.value != 0 else "")


def copy_from_device_address(dst, addr, nbytes):
    """Copy nbytes from a raw device address (as sp_read_gpu returns them: a float) into a torch CUDA tensor."""
    hip = C.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(int(addr)), C.c_size_t(int(nbytes)), C.c_int(3))   # device to device
    if rc != 0:
        raise BackendError("hipMemcpy failed: %d" % rc)


def sp_free_gpu(h):
    a, b, c, st = C.c_double(h["col_ptr"]), C.c_double(h["row_idx"]), C.c_double(h["values"]), C.c_int(-99)
    lib().rcppml_sp_free_gpu(C.byref(a), C.byref(b), C.byref(c), C.byref(st))
    h["col_ptr"], h["row_idx"], h["values"] = a.value, b.value, c.value
    return st.value


def nmf_dense(A, k, W_T, H, *, entry="float", max_iter=100, tol=1e-4, L1_H=0.0, L1_W=0.0, L2_H=0.0, L2_W=0.0, L21_H=0.0,
              L21_W=0.0, ortho_H=0.0, ortho_W=0.0, ub_H=0.0, ub_W=0.0, cd_maxit=100, verbose=0, seed=0, patience=5, nonneg_W=1,
              nonneg_H=1, loss_type=0, norm_type=0, projective=0, symmetric=0, solver_mode=0, robust_delta=0.0, irls_max_iter=5,
              irls_tol=1e-4, dispersion_mode=2, gp_theta_init=0.1, gp_theta_max=5.0, nb_size_init=10.0, nb_size_max=1e6,
              nb_size_min=0.01, tweedie_power=1.5):
    """Call the dense plugin entry as reference gpu/bridge_nmf.hpp:537-690 does.  A: (m, n) float64 array (any layout: it
    is handed over column-major).  W_T (m, k), H (n, k) float64, updated IN PLACE.  entry: "float" | "double"."""
    L = lib()
    A = np.asfortranarray(A, dtype=np.float64)
    m, n = A.shape
    assert W_T.dtype == np.float64 and H.dtype == np.float64 and W_T.flags.c_contiguous and H.flags.c_contiguous
    assert W_T.shape == (m, k) and H.shape == (n, k)
    d = np.ones(k, np.float64)
    theta = np.zeros(max(m, n, 1), np.float64)          # gpu/bridge_nmf.hpp:622 theta_buf(max(m, n))
    # (the build-defined entries read *out_theta_len on input as the capacity of out_theta)
    out_iter, out_conv, out_status, out_theta_len = C.c_int(0), C.c_int(0), C.c_int(-99), C.c_int((theta.shape[0] if theta_capacity is None else int(theta_capacity)) if entry == "ex" else 0)
    out_loss, out_tol = C.c_double(0), C.c_double(0)
    args = [
        A.ctypes.data_as(C.POINTER(C.c_double)), _ci(m), _ci(n), _ci(k), _np_ptr(W_T), _np_ptr(H), _np_ptr(d), _ci(max_iter), _cd(tol),
        _cd(L1_H), _cd(L1_W), _cd(L2_H), _cd(L2_W), _cd(L21_H), _cd(L21_W), _cd(ortho_H), _cd(ortho_W), _cd(ub_H), _cd(ub_W),
        _ci(cd_maxit), _ci(verbose), _ci(seed), _ci(1), _ci(patience), _ci(nonneg_W), _ci(nonneg_H), _ci(loss_type), _cd(1.0),
        _ci(irls_max_iter), _cd(irls_tol), _ci(norm_type), _ci(dispersion_mode), _cd(gp_theta_init), _cd(gp_theta_max), _cd(0.0),
        _cd(nb_size_init), _cd(nb_size_max), _cd(nb_size_min),
        _cd(robust_delta), _cd(tweedie_power), _ci(projective), _ci(symmetric), _ci(solver_mode), _np_ptr(theta), C.byref(out_theta_len),
        C.byref(out_iter), C.byref(out_conv), C.byref(out_loss), C.byref(out_status), C.byref(out_tol),
    ]
    assert len(args) == 50
    getattr(L, "rcppml_gpu_nmf_dense_unified_" + entry)(*args)
    return dict(d=d, iter=out_iter.value, converged=bool(out_conv.value), loss=out_loss.value, tol=out_tol.value,
                theta=theta[:out_theta_len.value].copy(), status=out_status.value, error=last_error() if out_status.value != 0 else "")


# ----------------------------------------------------------------------------- clustering (ops_cluster.hip)
def _csc_args(p, i, x):
    return (np.ascontiguousarray(p, np.int32), np.ascontiguousarray(i, np.int32), np.ascontiguousarray(x, np.float64))


def _matrix_head(csc, dense):
    """(col_ptr, row_idx, values, nnz, dense) of the entries that take either matrix form, and the arrays to keep alive.  csc: an
    object with p / i / x (data.CSC) or a (p, i, x) tuple, or None; dense: m x n (any order; handed over column-major) or None.
    None hands over null pointers."""
    keep = []
    if csc is not None:
        p, i, x = _csc_args(*((csc.p, csc.i, csc.x) if hasattr(csc, "p") else csc))
        keep += [p, i, x]
        head = [_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(x.shape[0])]
    else:
        head = [None, None, None, _ci(0)]
    if dense is not None:
        dn = np.asfortranarray(dense, np.float64)
        keep.append(dn)
        head.append(_np_ptr(dn))
    else:
        head.append(None)
    return head, keep


def bipartition_double(p, i, x, m, n, *, max_iter=100, tol=1e-5, nonneg=True, seed=0.0, partition=None, v=None, center=None):
    """The R-shaped 15-pointer entry (reference src/gpu_bridge_cluster.cu:57-62), with R's buffer sizes by default: partition n
    ints, v m doubles, center 2 m doubles (tests hand in larger buffers to watch what lies past them).  Returns dict(status,
    error, partition, v, center, dist)."""
    p, i, x = _csc_args(p, i, x)
    partition = np.zeros(n, np.int32) if partition is None else partition
    v = np.zeros(m, np.float64) if v is None else v
    center = np.zeros(2 * m, np.float64) if center is None else center
    dist, st = C.c_double(0.0), C.c_int(-99)
    lib().rcppml_gpu_bipartition_double(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(max_iter),
                                        _cd(tol), _ci(1 if nonneg else 0), _cd(seed), _np_ptr(partition), _np_ptr(v),
                                        _np_ptr(center), C.byref(dist), C.byref(st))
    return dict(status=st.value, error=last_error() if st.value else "", partition=partition, v=v, center=center, dist=dist.value)


def dclust_double(p, i, x, m, n, *, min_samples, min_dist=0.0, max_iter=100, tol=1e-5, nonneg=True, seed=0.0, max_clusters=0,
                  assignments=None):
    """The R-shaped 16-pointer entry (reference src/gpu_bridge_cluster.cu:105-110).  Returns dict(status, error, assignments,
    num_clusters)."""
    p, i, x = _csc_args(p, i, x)
    assignments = np.zeros(n, np.int32) if assignments is None else assignments
    nc, st = C.c_int(0), C.c_int(-99)
    lib().rcppml_gpu_dclust_double(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(max_clusters),
                                   _ci(min_samples), _cd(min_dist), _ci(max_iter), _cd(tol), _ci(1 if nonneg else 0), _cd(seed),
                                   _np_ptr(assignments), C.byref(nc), C.byref(st))
    return dict(status=st.value, error=last_error() if st.value else "", assignments=assignments, num_clusters=nc.value)


def bipartition_ex(p, i, x, m, n, samples=None, *, max_iter=100, tol=1e-5, nonneg=True, seed=0.0, calc_dist=True, capacity=None):
    """Build-defined bipartition of a sample subset (0-based, duplicates allowed).  capacity: (partition, v, center) buffer
    sizes to hand in (tests of the capacity check); default: what the call needs.  Returns dict(status, error, partition, v,
    center, size1, size2, dist, iter, needed)."""
    p, i, x = _csc_args(p, i, x)
    smp = None if samples is None else np.ascontiguousarray(samples, np.int32)
    ns = n if smp is None else smp.shape[0]
    caps = list(capacity) if capacity is not None else [ns, ns, 2 * m]
    part = np.zeros(max(caps[0], 1), np.int32)
    v = np.zeros(max(caps[1], 1), np.float64)
    center = np.zeros(max(caps[2], 1), np.float64)
    lens = [C.c_int(int(c)) for c in caps]
    s1, s2, it, st, dist = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(-99), C.c_double(0.0)
    lib().rcppml_gpu_bipartition_ex(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]),
                                    _np_ptr(smp) if smp is not None else None, _ci(0 if smp is None else ns), _ci(max_iter), _cd(tol),
                                    _ci(1 if nonneg else 0), _cd(seed), _ci(1 if calc_dist else 0), _np_ptr(part), C.byref(lens[0]),
                                    _np_ptr(v), C.byref(lens[1]), _np_ptr(center), C.byref(lens[2]), C.byref(s1), C.byref(s2),
                                    C.byref(dist), C.byref(it), C.byref(st))
    return dict(status=st.value, error=last_error() if st.value else "", partition=part[:ns], v=v[:ns], center=center[:2 * m],
                size1=s1.value, size2=s2.value, dist=dist.value, iter=it.value, needed=[l.value for l in lens])


def dclust_ex(p, i, x, m, n, *, min_samples, min_dist=0.0, max_iter=100, tol=1e-5, nonneg=True, seed=0.0, centers=True,
              cluster_cap=None, node_cap=None):
    """Build-defined dclust.  Without capacities the call is made with room for every tree the parameters allow: each cluster but
    a lone root holds at least min_samples samples, so there are at most max(1, n // min_samples) clusters and twice as many
    nodes.  Returns dict(status, error, assignments, size, radius, node, center (clusters x m or
    None), parent, bit, iter (per node), ids (binary path strings), clusters, nodes)."""
    p, i, x = _csc_args(p, i, x)
    bound = max(1, n // max(int(min_samples), 1))
    ccap = bound if cluster_cap is None else int(cluster_cap)
    ncap = 2 * bound if node_cap is None else int(node_cap)
    asg = np.zeros(n, np.int32)
    size = np.zeros(max(ccap, 1), np.int32)
    radius = np.zeros(max(ccap, 1), np.float64)
    node = np.zeros(max(ccap, 1), np.int32)
    center = np.zeros((max(ccap, 1), m), np.float64) if centers else None
    parent = np.zeros(max(ncap, 1), np.int32)
    bit = np.zeros(max(ncap, 1), np.int32)
    niter = np.zeros(max(ncap, 1), np.int32)
    cc, nc, st = C.c_int(ccap), C.c_int(ncap), C.c_int(-99)
    lib().rcppml_gpu_dclust_ex(_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(min_samples), _cd(min_dist),
                               _ci(max_iter), _cd(tol), _ci(1 if nonneg else 0), _cd(seed), _np_ptr(asg), C.byref(cc), _np_ptr(size),
                               _np_ptr(radius), _np_ptr(node), _np_ptr(center) if centers else None, C.byref(nc), _np_ptr(parent),
                               _np_ptr(bit), _np_ptr(niter), C.byref(st))
    out = dict(status=st.value, error=last_error() if st.value else "", clusters=cc.value, nodes=nc.value, assignments=asg)
    if st.value != 0:
        return out
    L, N = cc.value, nc.value
    parent, bit = parent[:N], bit[:N]
    paths = [""] * N
    for k in range(1, N):                 # children are appended after their parent: one pass in node order
        paths[k] = paths[parent[k]] + str(int(bit[k]))
    out.update(size=size[:L], radius=radius[:L], node=node[:L], center=center[:L] if centers else None, parent=parent, bit=bit,
               iter=niter[:N], ids=[paths[node[c]] for c in range(L)])
    return out


# ----------------------------------------------------------------------------- truncated SVD / PCA (ops_svd.hip)
SVD_ALGORITHMS = {"deflation": 0, "irlba": 1, "lanczos": 2, "randomized": 3, "krylov": 4}


def _svd_head(A, dense):
    """(the matrix arguments every SVD entry begins with, the arrays to keep alive, m, n).  A: (p, i, x, m, n) CSC parts, or an
    (m, n) array with dense=True (handed over column-major)."""
    if dense:
        Ad = np.asfortranarray(np.asarray(A, np.float64))
        m, n = Ad.shape
        return [_np_ptr(Ad.ravel(order="F")), _ci(m), _ci(n)], [Ad], m, n
    p, i, x, m, n = A
    p, i, x = _csc_args(p, i, x)
    return [_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0])], [p, i, x], m, n


def _svd_buffers(m, n, kb, buffers, **extra):
    """The output buffers of a call: U, d, V, row_means and the entry's further ones (name=size; iters holds ints), zeroed, with
    the caller's buffers in their place as they are."""
    sizes = dict(U=m * kb, d=kb, V=n * kb, row_means=m, **extra)
    b = {key: np.zeros(size, np.int32 if key == "iters" else np.float64) for key, size in sizes.items()}
    b.update(buffers or {})
    return b


def _svd_penalties(L1, L2, nonneg, upper_bound):
    """L1_u .. ub_v: the eight element-constraint arguments, in the order every entry takes them."""
    return [_cd(L1[0]), _cd(L1[1]), _cd(L2[0]), _cd(L2[1]), _ci(int(bool(nonneg[0]))), _ci(int(bool(nonneg[1]))),
            _cd(upper_bound[0]), _cd(upper_bound[1])]


def _svd_scalars(precision, k_max, tol, max_iter, center, seed, *penalties):
    """precision .. ub_v: the scalars a build-defined entry takes after the matrix (tol=None: the entry has no tol)."""
    return ([_ci(F32 if precision == "float" else F64), _ci(k_max)] + ([] if tol is None else [_cd(tol)]) +
            [_ci(max_iter), _ci(int(bool(center))), _ci(seed)] + _svd_penalties(*penalties))


def _svd_graph(g, keep, r_style=False):
    """The six arguments of one graph, (p, i, x, dim, lambda) or None.  None hands over null pointers, or with r_style the
    one-element arrays R hands over; a graph without entries keeps its col_ptr and hands over one-element arrays for the rest."""
    if g is None and not r_style:
        return [None] * 6
    gp, gi, gx, dim, lam = g if g is not None else ([0], [], [], 0, 0.0)
    gp, gi, gx = _csc_args(gp, gi, gx)
    gi_arg, gx_arg = (gi, gx) if gx.shape[0] else (np.zeros(1, np.int32), np.zeros(1))
    keep.extend([gp, gi_arg, gx_arg])
    return [_np_ptr(gp), _np_ptr(gi_arg), _np_ptr(gx_arg), _ci(dim), _ci(gx.shape[0]), _cd(lam)]


def _svd_mask(obs_mask, keep):
    """The five arguments of a pattern obs-mask, (p, i, rows, cols) or None (null pointers)."""
    if obs_mask is None:
        return [None] * 5
    op_, oi, rows, cols = obs_mask
    op_ = np.ascontiguousarray(op_, np.int32)
    oi = np.ascontiguousarray(oi, np.int32)
    oi_arg = oi if oi.shape[0] else np.zeros(1, np.int32)
    keep.extend([op_, oi_arg])
    return [_np_ptr(op_), _np_ptr(oi_arg), _ci(rows), _ci(cols), _ci(oi.shape[0])]


def _svd_result(st, b, m, n, kb, ksel, frob, wall, short_ok=False):
    """What every wrapper returns after its call: status and error, U (m x kb) and V (n x kb) as views of their buffers (short_ok:
    a buffer too short for that comes back as it is), d, k, frob, row_means, wall_ms and the buffers."""
    U, V = (b[key] if short_ok and b[key].size < rows * kb else b[key][:rows * kb].reshape(kb, rows).T
            for key, rows in (("U", m), ("V", n)))
    return dict(status=st.value, error=last_error() if st.value else "", U=U, V=V, d=b["d"], k=ksel.value, frob=frob.value,
                row_means=b["row_means"], wall_ms=wall.value, buffers=b)


def svd_pca(A, k_max, *, dense=False, precision="double", tol=1e-5, max_iter=200, center=False, seed=0, L1=(0.0, 0.0),
            L2=(0.0, 0.0), nonneg=(False, False), upper_bound=(0.0, 0.0), L21=(0.0, 0.0), angular=(0.0, 0.0), test_fraction=0.0,
            algorithm=0, graph_u=None, graph_v=None, obs_mask=None, robust_delta=0.0, buffers=None):
    """One of the four R-shaped entries (reference src/gpu_bridge_svd.cu), with the arguments laid out as R's .gpu_svd_pca /
    .gpu_svd_pca_dense pass them (R/gpu_backend.R:295-420).  A: (p, i, x, m, n) CSC parts, or a column-major (m, n) array with
    dense=True.  graph_u / graph_v: (p, i, x, dim, lambda); obs_mask: (p, i, x, rows, cols).  buffers: dict of preallocated outputs
    (tests watch what is left untouched).  Returns dict(status, error, U (m x k_max), d, V (n x k_max), k, iters, frob, row_means,
    wall_ms, test_loss)."""
    head, keep, m, n = _svd_head(A, dense)
    b = _svd_buffers(m, n, k_max, buffers, test_loss=k_max, iters=k_max)      # R sizes them by k_max itself
    op_, oi, ox, rows, cols = obs_mask if obs_mask is not None else ([0], [0], [0.0], 0, 0)      # or R's one-element placeholders
    op_, oi, ox = _csc_args(op_, oi, ox)
    keep.extend([op_, oi, ox])
    ksel, wall, frob, st = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    args = head + [_ci(k_max), _np_ptr(b["U"]), _np_ptr(b["d"]), _np_ptr(b["V"]), _cd(tol), _ci(max_iter), _ci(int(bool(center))),
                   _ci(0), _ci(seed), _ci(0)] + _svd_penalties(L1, L2, nonneg, upper_bound) + [
                   _cd(L21[0]), _cd(L21[1]), _cd(angular[0]), _cd(angular[1]), _cd(test_fraction), _ci(0), _ci(5), _ci(0),
                   _ci(algorithm)] + _svd_graph(graph_u, keep, r_style=True) + _svd_graph(graph_v, keep, r_style=True) + [
                   _np_ptr(op_), _np_ptr(oi), _np_ptr(ox), _ci(rows), _ci(cols), _ci(ox.shape[0] if obs_mask is not None else 0),
                   C.byref(ksel), C.byref(wall), _np_ptr(b["test_loss"]), _np_ptr(b["iters"]), C.byref(frob), _np_ptr(b["row_means"]),
                   _cd(robust_delta), _ci(5), _cd(1e-4), C.byref(st)]
    assert len(args) == (58 if dense else 61)
    name = "rcppml_gpu_svd_pca_" + ("dense_" if dense else "") + ("float" if precision == "float" else "double")
    getattr(lib(), name)(*args)
    return dict(_svd_result(st, b, m, n, k_max, ksel, frob, wall), iters=b["iters"], test_loss=b["test_loss"])


def svd_cv(A, k_max, *, dense=False, precision="double", tol=1e-5, max_iter=200, center=False, seed=0, L1=(0.0, 0.0),
           L2=(0.0, 0.0), nonneg=(False, False), upper_bound=(0.0, 0.0), test_fraction=0.0, cv_seed=0, patience=3, mask_zeros=False,
           obs_mask=None, buffers=None):
    """The build-defined rcppml_gpu_svd_cv_ex / rcppml_gpu_svd_cv_dense_ex: cross-validated / auto-rank and obs-masked deflation.
    A as in svd_pca; obs_mask: (p, i, rows, cols) pattern CSC or None.  buffers: dict of preallocated outputs.  Returns dict(status,
    error, U (m x k_max), d, V (n x k_max), k (selected), k_computed, test_loss, n_test, n_masked, iters, frob, row_means, wall_ms)."""
    head, keep, m, n = _svd_head(A, dense)
    kb = max(k_max, 1)
    b = _svd_buffers(m, n, kb, buffers, test_loss=kb, iters=kb)
    ksel, kcomp, ntest, nmask = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    wall, frob, st = C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    args = head + _svd_scalars(precision, k_max, tol, max_iter, center, seed, L1, L2, nonneg, upper_bound) + [
        _cd(test_fraction), _ci(cv_seed), _ci(patience), _ci(int(bool(mask_zeros)))] + _svd_mask(obs_mask, keep) + [
        _np_ptr(b["U"]), _np_ptr(b["d"]), _np_ptr(b["V"]), C.byref(ksel), C.byref(kcomp), _np_ptr(b["test_loss"]), C.byref(ntest),
        C.byref(nmask), _np_ptr(b["iters"]), C.byref(frob), _np_ptr(b["row_means"]), C.byref(wall), C.byref(st)]
    assert len(args) == (39 if dense else 42)
    getattr(lib(), "rcppml_gpu_svd_cv_dense_ex" if dense else "rcppml_gpu_svd_cv_ex")(*args)
    return dict(_svd_result(st, b, m, n, kb, ksel, frob, wall), k_computed=kcomp.value, test_loss=b["test_loss"],
                n_test=ntest.value, n_masked=nmask.value, iters=b["iters"])


def svd_reg(A, k_max, *, dense=False, precision="double", tol=1e-5, max_iter=200, center=False, seed=0, L1=(0.0, 0.0),
            L2=(0.0, 0.0), nonneg=(False, False), upper_bound=(0.0, 0.0), L21=(0.0, 0.0), angular=(0.0, 0.0), graph_u=None,
            graph_v=None, test_fraction=0.0, cv_seed=0, patience=3, mask_zeros=False, obs_mask=None, buffers=None):
    """The build-defined rcppml_gpu_svd_reg_ex / rcppml_gpu_svd_reg_dense_ex: svd_cv plus L21, angular and graph regularisation in
    the deflation loop.  A, obs_mask, buffers and the result dict as in svd_cv; L21 / angular: (u, v); graph_u / graph_v: (p, i, x,
    dim, lambda) as svd_pca takes them, or None."""
    head, keep, m, n = _svd_head(A, dense)
    kb = max(k_max, 1)
    b = _svd_buffers(m, n, kb, buffers, test_loss=kb, iters=kb)
    ksel, kcomp, ntest, nmask = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    wall, frob, st = C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    args = head + _svd_scalars(precision, k_max, tol, max_iter, center, seed, L1, L2, nonneg, upper_bound) + [
        _cd(L21[0]), _cd(L21[1]), _cd(angular[0]), _cd(angular[1])] + _svd_graph(graph_u, keep) + _svd_graph(graph_v, keep) + [
        _cd(test_fraction), _ci(cv_seed), _ci(patience), _ci(int(bool(mask_zeros)))] + _svd_mask(obs_mask, keep) + [
        _np_ptr(b["U"]), _np_ptr(b["d"]), _np_ptr(b["V"]), C.byref(ksel), C.byref(kcomp), _np_ptr(b["test_loss"]), C.byref(ntest),
        C.byref(nmask), _np_ptr(b["iters"]), C.byref(frob), _np_ptr(b["row_means"]), C.byref(wall), C.byref(st)]
    assert len(args) == (55 if dense else 58)
    getattr(lib(), "rcppml_gpu_svd_reg_dense_ex" if dense else "rcppml_gpu_svd_reg_ex")(*args)
    return dict(_svd_result(st, b, m, n, kb, ksel, frob, wall), k_computed=kcomp.value, test_loss=b["test_loss"],
                n_test=ntest.value, n_masked=nmask.value, iters=b["iters"])


def krylov_pass_limit(k, max_iter=0):
    """krylov.hpp:428-431: the pass limit of KSPR at rank k."""
    return int(max_iter) if max_iter > 0 else max(10, 2 * int(np.ceil(np.log2(max(k, 1)))) + 3)


def svd_krylov(A, k_max, *, dense=False, precision="double", tol=1e-5, max_iter=0, center=False, seed=0, L1=(0.0, 0.0), L2=(0.0, 0.0),
               nonneg=(False, False), upper_bound=(0.0, 0.0), V0=None, buffers=None):
    """The build-defined rcppml_gpu_svd_krylov_ex / rcppml_gpu_svd_krylov_dense_ex: the constrained block SVD (KSPR).  A as in
    svd_pca; V0: n x k_max seed or None (Lanczos).  buffers: dict of preallocated outputs.  Returns dict(status, error, U (m x k_max),
    d, V (n x k_max), k (k_actual), passes, dw (passes - 1 values), frob, row_means, wall_ms)."""
    head, keep, m, n = _svd_head(A, dense)
    kb = max(k_max, 1)
    b = _svd_buffers(m, n, kb, buffers, dw=krylov_pass_limit(kb, max_iter))
    v0 = None
    if V0 is not None:
        v0 = np.asfortranarray(np.asarray(V0, np.float64))
        assert v0.shape == (n, k_max), "V0 must be n x k_max"
        keep.append(v0)
    ksel, passes = C.c_int(0), C.c_int(0)
    wall, frob, st = C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    args = head + _svd_scalars(precision, k_max, tol, max_iter, center, seed, L1, L2, nonneg, upper_bound) + [
        _np_ptr(v0.ravel(order="F")) if v0 is not None else None, _np_ptr(b["U"]), _np_ptr(b["d"]), _np_ptr(b["V"]), C.byref(ksel),
        C.byref(passes), _np_ptr(b["dw"]), C.byref(frob), _np_ptr(b["row_means"]), C.byref(wall), C.byref(st)]
    assert len(args) == (28 if dense else 31)
    getattr(lib(), "rcppml_gpu_svd_krylov_dense_ex" if dense else "rcppml_gpu_svd_krylov_ex")(*args)
    return dict(_svd_result(st, b, m, n, kb, ksel, frob, wall), passes=passes.value, dw=b["dw"][:max(passes.value - 1, 0)])


RANDOMIZED_MAX_SKETCH = 128


def randomized_sizes(m, n, k, max_iter=0):
    """randomized.hpp:73-76: (oversampling p, sketch dimension l, power iterations q) of the randomized method."""
    p = min(max(10, k // 5), min(m, n) - k)
    return p, k + max(p, 0), 3 if max_iter <= 0 else min(int(max_iter), 10)


def svd_randomized(A, k_max, *, dense=False, precision="double", max_iter=0, center=False, seed=0, buffers=None, L1=(0.0, 0.0),
                   L2=(0.0, 0.0), nonneg=(False, False), upper_bound=(0.0, 0.0), L21=(0.0, 0.0), angular=(0.0, 0.0), graph_u=None,
                   graph_v=None, test_fraction=0.0, obs_mask=None):
    """The build-defined rcppml_gpu_svd_randomized_ex / rcppml_gpu_svd_randomized_dense_ex: the randomized block SVD
    (Halko-Martinsson-Tropp).  A as in svd_pca; max_iter: the power iterations q (<= 0: 3, at most 10).  buffers: dict of
    preallocated outputs.  Everything after buffers is what the method does not support and the entry refuses: graph_u / graph_v:
    (p, lambda) or None, obs_mask: a column-pointer array or None.  Returns the dict of svd_pca: status, error, U (m x k_max), d,
    V (n x k_max), k, iters, frob, row_means, wall_ms, test_loss (empty)."""
    head, keep, m, n = _svd_head(A, dense)
    kb = max(k_max, 1)
    b = _svd_buffers(m, n, kb, buffers, iters=kb)       # a buffer handed in is used as it is (a refused call may get a short one)

    def graph(g):
        if g is None:
            return [None, _cd(0.0)]
        gp = np.ascontiguousarray(g[0], np.int32)
        keep.append(gp)
        return [_np_ptr(gp), _cd(g[1])]

    om = None
    if obs_mask is not None:
        om = np.ascontiguousarray(obs_mask, np.int32)
        keep.append(om)
    ksel, wall, frob, st = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    args = head + _svd_scalars(precision, k_max, None, max_iter, center, seed, L1, L2, nonneg, upper_bound) + [
        _cd(L21[0]), _cd(L21[1]), _cd(angular[0]), _cd(angular[1])] + graph(graph_u) + graph(graph_v) + [
        _cd(test_fraction), _np_ptr(om) if om is not None else None, _np_ptr(b["U"]), _np_ptr(b["d"]), _np_ptr(b["V"]),
        C.byref(ksel), _np_ptr(b["iters"]), C.byref(frob), _np_ptr(b["row_means"]), C.byref(wall), C.byref(st)]
    assert len(args) == (35 if dense else 38)
    getattr(lib(), "rcppml_gpu_svd_randomized_dense_ex" if dense else "rcppml_gpu_svd_randomized_ex")(*args)
    return dict(_svd_result(st, b, m, n, kb, ksel, frob, wall, short_ok=True), iters=b["iters"], test_loss=np.zeros(0))


def nmf_svd_init(A, k, *, dense=False, precision="double", seed=0, mode=1, buffers=None):
    """The build-defined rcppml_gpu_nmf_svd_init_ex / rcppml_gpu_nmf_svd_init_dense_ex: the SVD-seeded start of an NMF fit
    (nmf/nmf_init.hpp:45-158).  A as in svd_pca; seed: the uint32 the reference's config carries; mode: 1 Lanczos, 2 IRLBA (the same
    engine).  buffers: dict of preallocated outputs W_T (m * k), H (n * k), d (k).  Returns dict(status, error, W_T ((m, k) C-order:
    the column-major k x m the fit entries take), H ((n, k)), d (k_svd values), k_svd, iters, wall_ms, buffers)."""
    head, keep, m, n = _svd_head(A, dense)
    kb = max(k, 1)
    b = dict(W_T=np.zeros(m * kb), H=np.zeros(n * kb), d=np.zeros(kb))
    b.update(buffers or {})
    ksvd, iters, wall, st = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_int(-99)
    args = head + [_ci(F32 if precision == "float" else F64), _ci(k), C.byref(C.c_int(int(seed) & 0xFFFFFFFF)), _ci(mode),
                   _np_ptr(b["W_T"]), _np_ptr(b["H"]), _np_ptr(b["d"]), C.byref(ksvd), C.byref(iters), C.byref(wall), C.byref(st)]
    assert len(args) == (14 if dense else 17)
    getattr(lib(), "rcppml_gpu_nmf_svd_init_dense_ex" if dense else "rcppml_gpu_nmf_svd_init_ex")(*args)
    full = b["W_T"].size >= m * kb and b["H"].size >= n * kb
    return dict(status=st.value, error=last_error() if st.value else "", W_T=b["W_T"][:m * kb].reshape(m, kb) if full else b["W_T"],
                H=b["H"][:n * kb].reshape(n, kb) if full else b["H"], d=b["d"][:ksvd.value], k_svd=ksvd.value, iters=iters.value,
                wall_ms=wall.value, buffers=b)


def nmf_start_time(length, ja, kc, k, *, precision="double", reps=20):
    """rcppml_hip_nmf_start_time: (ms of one nmf_start_kernel launch, ms of the one ritz_kernel launch it replaces), medians of
    `reps` launches on a length x ja basis with kc of k columns wanted."""
    a, b, st = C.c_double(0.0), C.c_double(0.0), C.c_int(-99)
    lib().rcppml_hip_nmf_start_time(_ci(F32 if precision == "float" else F64), _ci(length), _ci(ja), _ci(kc), _ci(k), _ci(reps),
                                    C.byref(a), C.byref(b), C.byref(st))
    if st.value != 0:
        raise BackendError("rcppml_hip_nmf_start_time failed: %s" % last_error())
    return a.value, b.value


# ----------------------------------------------------------------------------- embedding assessment (ops_assess.hip)
KNN_MASK = {"none": 0, "self": 1, "group": 2}
_ASSESS_OUT = ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy")


def _assess_head(emb, labels, n_classes, batch, n_batch, flags, nstart, maxiter, spc, knn_k, folds, batch_k, seed, outs):
    e = np.ascontiguousarray(emb, np.float64)
    n, dim = (e.shape if e.ndim == 2 else (int(e.shape[0]), 1))
    lab = np.ascontiguousarray(np.zeros(n) if labels is None else labels, np.int32)
    bat = np.ascontiguousarray(np.full(n, -1) if batch is None else batch, np.int32)
    args = [_np_ptr(e), _ci(n), _ci(dim), _np_ptr(lab), _ci(n_classes), _np_ptr(bat), _ci(n_batch)] + [_ci(int(bool(f))) for f in flags] + [
        _ci(nstart), _ci(maxiter), _ci(spc), _ci(knn_k), _ci(folds), _ci(batch_k), _ci(seed)] + [C.byref(o) for o in outs]
    return args, (e, lab, bat), n


def assess_raw(emb, labels, n_classes, batch=None, n_batch=0, *, clustering=True, silhouette=True, classify=True, batch_mixing=True,
               nstart=10, maxiter=100, spc=200, knn_k=15, folds=5, batch_k=50, seed=42, init=0.0):
    """The R-shaped 26-pointer entry (reference src/gpu_bridge_assess.cu:358-376), laid out as R's .assess_gpu passes it
    (R/assess.R:708-769).  emb: n x dim (row-major doubles are handed over).  The seven outputs start at `init` (what is not computed
    stays so).  Returns dict(status, error, ari, nmi, silhouette, knn_accuracy, knn_f1, batch_sil, batch_entropy)."""
    outs = [C.c_double(init) for _ in _ASSESS_OUT]
    args, keep, n = _assess_head(emb, labels, n_classes, batch, n_batch, (clustering, silhouette, classify, batch_mixing), nstart,
                                 maxiter, spc, knn_k, folds, batch_k, seed, outs)
    st = C.c_int(-99)
    args.append(C.byref(st))
    assert len(args) == 26
    lib().rcppml_gpu_assess(*args)
    r = dict(status=st.value, error=last_error() if st.value else "")
    r.update({k: o.value for k, o in zip(_ASSESS_OUT, outs)})
    return r


def assess_ex(emb, labels, n_classes, batch=None, n_batch=0, *, clustering=True, silhouette=True, classify=True, batch_mixing=True,
              nstart=10, maxiter=100, spc=200, knn_k=15, folds=5, batch_k=50, seed=42, init=0.0, capacity=None):
    """Build-defined rcppml_gpu_assess_ex: the 26-pointer results plus assignments (best restart), restart_ari / restart_nmi,
    sil_point (fp32), fold_ids, fold_accuracy / fold_f1 (NaN: fold without training or test points), batch_entropy_point,
    batch_sil_point.  capacity: (point, restart, fold) buffer lengths to hand in; default: what the call needs."""
    outs = [C.c_double(init) for _ in _ASSESS_OUT]
    args, keep, n = _assess_head(emb, labels, n_classes, batch, n_batch, (clustering, silhouette, classify, batch_mixing), nstart,
                                 maxiter, spc, knn_k, folds, batch_k, seed, outs)
    caps = list(capacity) if capacity is not None else [n, max(nstart, 0), max(folds, 0)]
    b = dict(assignments=np.full(max(caps[0], 1), -7, np.int32), restart_ari=np.full(max(caps[1], 1), np.nan),
             restart_nmi=np.full(max(caps[1], 1), np.nan), sil_point=np.full(max(caps[0], 1), np.nan, np.float32),
             fold_ids=np.full(max(caps[0], 1), -7, np.int32), fold_accuracy=np.full(max(caps[2], 1), -7.0),
             fold_f1=np.full(max(caps[2], 1), -7.0), batch_entropy_point=np.full(max(caps[0], 1), np.nan),
             batch_sil_point=np.full(max(caps[0], 1), np.nan))
    order = ("assignments", "restart_ari", "restart_nmi", "sil_point", "fold_ids", "fold_accuracy", "fold_f1", "batch_entropy_point",
             "batch_sil_point")
    st = C.c_int(-99)
    args += [_np_ptr(b[k]) for k in order] + [_ci(c) for c in caps] + [C.byref(st)]
    lib().rcppml_gpu_assess_ex(*args)
    r = dict(status=st.value, error=last_error() if st.value else "")
    r.update({k: o.value for k, o in zip(_ASSESS_OUT, outs)})
    lens = dict(assignments=n, restart_ari=max(nstart, 0), restart_nmi=max(nstart, 0), sil_point=n, fold_ids=n,
                fold_accuracy=max(folds, 0), fold_f1=max(folds, 0), batch_entropy_point=n, batch_sil_point=n)
    r.update({k: b[k][:lens[k]] for k in order})
    r["buffers"] = b
    return r


def knn_float(query, train=None, k=15, *, mask="none", group=None, group_k=None, capacity=None):
    """rcppml_gpu_knn_float: exact fp32 brute-force kNN.  query (nq x dim) / train (nt x dim, None: the query matrix itself, which
    mask "self" and "group" need).  group: nq ints, group_k: k per group (mask "group").  Returns dict(status, error, idx (nq x k,
    -1 = empty), dist (nq x k float32, 1e30 = empty))."""
    q = np.ascontiguousarray(query, np.float32)
    if q.ndim == 1:
        q = q[:, None]
    nq, dim = q.shape
    t = None if train is None else np.ascontiguousarray(train, np.float32).reshape(-1, dim)
    g = None if group is None else np.ascontiguousarray(group, np.int32)
    gk = None if group_k is None else np.ascontiguousarray(group_k, np.int32)
    ng = 0 if g is None else (int(g.max()) + 1 if g.size else 0)
    if gk is not None:
        ng = max(ng, gk.shape[0])
    cap = nq * k if capacity is None else int(capacity)
    oi = np.full(max(cap, 1), -7, np.int32)
    od = np.full(max(cap, 1), np.nan, np.float32)
    st = C.c_int(-99)
    lib().rcppml_gpu_knn_float(_np_ptr(q), _ci(nq), _np_ptr(t) if t is not None else None, _ci(0 if t is None else t.shape[0]), _ci(dim),
                               _ci(k), _ci(KNN_MASK[mask]), _np_ptr(g) if g is not None else None,
                               _np_ptr(gk) if gk is not None else None, _ci(ng), _np_ptr(oi), _np_ptr(od), _ci(cap), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(oi, od))
    if st.value == 0:
        r.update(idx=oi[:nq * k].reshape(nq, k), dist=od[:nq * k].reshape(nq, k))
    return r


def assess_plan(labels, n_classes, *, nstart=10, spc=200, folds=5, seed=42, capacity=None):
    """rcppml_gpu_assess_plan (host only, no device): dict(status, error, init (nstart x n_classes point indices), sil_counts
    (n_classes, min(spc, size)), sil_samples (class by class), fold_ids (n))."""
    lab = np.ascontiguousarray(labels, np.int32)
    n = lab.shape[0]
    counts_max = int(np.sum(np.minimum(np.maximum(spc, 0), np.bincount(lab[(lab >= 0) & (lab < max(n_classes, 1))],
                                                                           minlength=max(n_classes, 1)))))
    caps = list(capacity) if capacity is not None else [max(nstart, 0) * max(n_classes, 0), counts_max, n]
    init = np.full(max(caps[0], 1), -7, np.int32)
    samples = np.full(max(caps[1], 1), -7, np.int32)
    counts = np.full(max(n_classes, 1), -7, np.int32)
    folds_out = np.full(max(caps[2], 1), -7, np.int32)
    st = C.c_int(-99)
    lib().rcppml_gpu_assess_plan(_np_ptr(lab), _ci(n), _ci(n_classes), _ci(nstart), _ci(spc), _ci(folds), _ci(seed), _np_ptr(init),
                                 _ci(caps[0]), _np_ptr(samples), _np_ptr(counts), _ci(caps[1]), _np_ptr(folds_out), _ci(caps[2]),
                                 C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(init, samples, counts, folds_out))
    if st.value == 0:
        tot = int(np.sum(np.maximum(counts[:n_classes], 0)))
        r.update(init=init[:max(nstart, 0) * n_classes].reshape(max(nstart, 0), n_classes), sil_counts=counts[:n_classes].copy(),
                 sil_samples=samples[:tot].copy(), fold_ids=folds_out[:n].copy())
    return r


# ----------------------------------------------------------------------------- classifier evaluation (ops_classify.hip)
CLASSIFY_DISTANCE = {"euclidean": 0, "cosine": 1}
_METRIC_OUT = ("predictions", "confusion", "precision", "recall", "f1", "support", "auc")


def _metric_buffers(n_test, C, init):
    nt, c = max(int(n_test), 1), max(int(C), 1)
    return dict(predictions=np.full(nt, int(init), np.int32), confusion=np.full(c * c, int(init), np.int32), precision=np.full(c, init),
                recall=np.full(c, init), f1=np.full(c, init), support=np.full(c, int(init), np.int32), auc=np.full(c, init))


def _rows(a):
    a = np.ascontiguousarray(a, np.float64)
    return a[:, None] if a.ndim == 1 else a


def classify_metrics(prob, test_labels, n_classes, *, init=-7.0, buffers=None):
    """rcppml_gpu_classify_metrics_ex.  prob: n_test x n_classes.  Returns dict(status, error, predictions, confusion (C x C, rows
    true), precision, recall, f1, support, auc (per class), buffers).  The outputs start at `init`; a refused call leaves them so."""
    pr = _rows(prob)
    tl = np.ascontiguousarray(test_labels, np.int32)
    nt, Cn = tl.shape[0], int(n_classes)
    if pr.shape != (nt, max(Cn, 1)) and Cn >= 1:
        raise ValueError("prob must be n_test x n_classes")
    b = buffers if buffers is not None else _metric_buffers(nt, Cn, init)
    return _classify_call("rcppml_gpu_classify_metrics_ex", [_np_ptr(pr), _np_ptr(tl), _ci(nt), _ci(Cn)], b, _METRIC_OUT, [], nt, Cn,
                          {}, (pr, tl))


def _classify_call(name, head, b, order, tail, nt, Cn, extra_shapes, keep):
    """keep: the input arrays, alive until the call returns."""
    st = C.c_int(-99)
    getattr(lib(), name)(*(head + [_np_ptr(b[k]) for k in order] + tail + [C.byref(st)]))
    shapes = dict(predictions=(nt,), confusion=(Cn, Cn), precision=(Cn,), recall=(Cn,), f1=(Cn,), support=(Cn,), auc=(Cn,))
    shapes.update(extra_shapes)
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=b)
    if st.value == 0:
        for k, shp in shapes.items():
            r[k] = b[k][:int(np.prod(shp))].reshape(shp).copy()
    return r


def _classify_head(train, test, train_labels, test_labels, n_classes):
    tr, te = _rows(train), _rows(test)
    ltr, lte = np.ascontiguousarray(train_labels, np.int32), np.ascontiguousarray(test_labels, np.int32)
    ntr, nte, dim = tr.shape[0], te.shape[0], tr.shape[1]
    if te.shape[1] != dim or ltr.shape != (ntr,) or lte.shape != (nte,):
        raise ValueError("train and test must have the same columns, and one label per row")
    head = [_np_ptr(tr), _np_ptr(te), _np_ptr(ltr), _np_ptr(lte), _ci(ntr), _ci(nte), _ci(dim), _ci(n_classes)]
    return head, (tr, te, ltr, lte), ntr, nte, dim


def classify_knn(train, test, train_labels, test_labels, n_classes, k=5, distance="euclidean", *, init=-7.0, buffers=None):
    """rcppml_gpu_classify_knn_ex: votes (n_test x C, neighbour label counts / k) and the metrics of classify_metrics, plus
    launches.  distance: "euclidean" / "cosine" (or the raw code)."""
    head, keep, ntr, nte, dim = _classify_head(train, test, train_labels, test_labels, n_classes)
    Cn = int(n_classes)
    b = buffers
    if b is None:
        b = _metric_buffers(nte, Cn, init)
        b["votes"] = np.full(max(nte, 1) * max(Cn, 1), init)
    launches = C.c_int(0)
    head += [_ci(k), _ci(CLASSIFY_DISTANCE.get(distance, distance))]
    r = _classify_call("rcppml_gpu_classify_knn_ex", head, b, ("votes",) + _METRIC_OUT, [C.byref(launches)], nte, Cn,
                       dict(votes=(nte, Cn)), keep)
    r["launches"] = launches.value
    return r


def classify_logistic(train, test, train_labels, test_labels, n_classes, maxit=25, epsilon=1e-8, *, row_blocks=0, init=-7.0,
                      buffers=None):
    """rcppml_gpu_classify_logistic_ex: coef (C x (dim + 1), intercept first), aliased, iters, converged, deviance (per class), prob
    (n_test x C, row-normalised) and the metrics of classify_metrics, plus launches.  row_blocks: the workgroups of the
    per-iteration pass (0: one per 128-row chunk); a test switch, the results do not depend on it."""
    head, keep, ntr, nte, dim = _classify_head(train, test, train_labels, test_labels, n_classes)
    Cn = int(n_classes)
    P = dim + 1
    b = buffers
    if b is None:
        b = _metric_buffers(nte, Cn, init)
        c1 = max(Cn, 1)
        b.update(coef=np.full(c1 * P, init), aliased=np.full(c1 * P, int(init), np.int32), iters=np.full(c1, int(init), np.int32),
                 converged=np.full(c1, int(init), np.int32), deviance=np.full(c1, init), prob=np.full(max(nte, 1) * c1, init))
    launches = C.c_int(0)
    head += [_ci(maxit), _cd(epsilon), _ci(row_blocks)]
    order = ("coef", "aliased", "iters", "converged", "deviance", "prob") + _METRIC_OUT
    r = _classify_call("rcppml_gpu_classify_logistic_ex", head, b, order, [C.byref(launches)], nte, Cn,
                       dict(coef=(Cn, P), aliased=(Cn, P), iters=(Cn,), converged=(Cn,), deviance=(Cn,), prob=(nte, Cn)), keep)
    r["launches"] = launches.value
    return r


# ----------------------------------------------------------------------------- distribution diagnostics (ops_distribution.hip)
def _dist_head(csc, dense, m, n, k, W_T, d, H):
    """The shared head (col_ptr, row_idx, values, nnz, dense, m, n, k, W_T, d, H) and the arrays to keep alive.  csc / dense as in
    _matrix_head.  W_T: (m, k) row-major (= k x m), d: (k), H: (n, k) row-major (= k x n)."""
    head, keep = _matrix_head(csc, dense)
    W_T = np.ascontiguousarray(W_T, np.float64); d = np.ascontiguousarray(d, np.float64); H = np.ascontiguousarray(H, np.float64)
    keep += [W_T, d, H]
    head += [_ci(m), _ci(n), _ci(k), _np_ptr(W_T), _np_ptr(d), _np_ptr(H)]
    return head, keep


def score_test_double(csc, dense, m, n, k, W_T, d, H, powers, min_mu=1e-6, init=-7.0):
    """rcppml_gpu_score_test_double: dict(status, error, T (per power), T_nb, all_integer, count, buffers).  Outputs start at `init`
    (a refused call leaves them so)."""
    head, keep = _dist_head(csc, dense, m, n, k, W_T, d, H)
    pw = np.ascontiguousarray(powers, np.float64).reshape(-1)
    T = np.full(max(pw.shape[0], 1), init)
    tnb, allint, cnt, st = C.c_double(init), C.c_int(-7), C.c_int64(-7), C.c_int(-99)
    lib().rcppml_gpu_score_test_double(*head, _np_ptr(pw), _ci(pw.shape[0]), _cd(min_mu), _np_ptr(T), C.byref(tnb), C.byref(allint),
                                       C.byref(cnt), C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(T, tnb.value, allint.value, cnt.value))
    if st.value == 0:
        r.update(T=T[:pw.shape[0]].copy(), T_nb=tnb.value, all_integer=bool(allint.value), count=int(cnt.value))
    return r


def zero_inflation_double(csc, dense, m, n, k, W_T, d, H, init=-7.0):
    """rcppml_gpu_zero_inflation_double: dict(status, error, expected_row, expected_col, observed_row, observed_col, buffers)."""
    head, keep = _dist_head(csc, dense, m, n, k, W_T, d, H)
    bufs = [np.full(max(v, 1), init) for v in (m, n, m, n)]
    st = C.c_int(-99)
    lib().rcppml_gpu_zero_inflation_double(*head, *[_np_ptr(b) for b in bufs], C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=bufs)
    if st.value == 0:
        r.update(expected_row=bufs[0][:m].copy(), expected_col=bufs[1][:n].copy(), observed_row=bufs[2][:m].copy(),
                 observed_col=bufs[3][:n].copy())
    return r


def dispersion_double(csc, dense, m, n, k, W_T, d, H, power, min_mu=1e-6, trim=0.1, init=-7.0):
    """rcppml_gpu_dispersion_double: dict(status, error, row_phi (m), col_phi (n), global_phi, buffers)."""
    head, keep = _dist_head(csc, dense, m, n, k, W_T, d, H)
    rp, cp, gp = np.full(max(m, 1), init), np.full(max(n, 1), init), C.c_double(init)
    st = C.c_int(-99)
    lib().rcppml_gpu_dispersion_double(*head, _cd(power), _cd(min_mu), _cd(trim), _np_ptr(rp), _np_ptr(cp), C.byref(gp), C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(rp, cp, gp.value))
    if st.value == 0:
        r.update(row_phi=rp[:m].copy(), col_phi=cp[:n].copy(), global_phi=gp.value)
    return r


# ----------------------------------------------------------------------------- consensus clustering (ops_consensus.hip)
CONSENSUS_METHOD = {"hard": 0, "knn_jaccard": 1}


def consensus_double(W_stack, m, k, reps, method, knn=10, *, labels=True, init=-7.0):
    """rcppml_gpu_consensus_double: dict(status, error, consensus (m x m), labels (reps x m, hard with labels=True), buffers).
    W_stack: (reps, m, k) C-contiguous (each replicate k x m column-major), or None (a null pointer).  method: 0 / 1 or a name of
    CONSENSUS_METHOD.  Outputs start at `init` / -7 (a refused call leaves them so)."""
    W = None if W_stack is None else np.ascontiguousarray(W_stack, np.float64)
    method = CONSENSUS_METHOD.get(method, method)
    mm, rr = max(int(m), 1), max(int(reps), 1)
    cons = np.full((mm, mm), init)
    lab = np.full((rr, mm), -7, np.int32) if labels else None
    st = C.c_int(-99)
    lib().rcppml_gpu_consensus_double(_np_ptr(W) if W is not None else None, _ci(m), _ci(k), _ci(reps), _ci(method), _ci(knn),
                                      _np_ptr(cons), _np_ptr(lab) if lab is not None else None, C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(cons,) if lab is None else (cons, lab))
    if st.value == 0:
        r.update(consensus=cons, labels=lab if (lab is not None and method == 0) else None)
    return r


def hclust_average_double(dist, k_cut, *, m=None, init=-7.0):
    """rcppml_gpu_hclust_average_double (host only, no device): dict(status, error, merge ((m - 1) x 2, R's convention), height
    (m - 1), clusters (m, numbered 1.. by first appearance), cophenetic, buffers).  dist: m x m, the entries below the diagonal are
    read (dist[i, j] with i > j), or None (a null pointer)."""
    D = None if dist is None else np.asfortranarray(dist, np.float64)
    if m is None:
        m = D.shape[0]
    mm = max(int(m), 2)
    merge = np.full((mm - 1, 2), -7, np.int32, order="F")
    height = np.full(mm - 1, init)
    clusters = np.full(mm, -7, np.int32)
    coph, st = C.c_double(init), C.c_int(-99)
    lib().rcppml_gpu_hclust_average_double(_np_ptr(D) if D is not None else None, _ci(m), _ci(k_cut), _np_ptr(merge), _np_ptr(height),
                                           _np_ptr(clusters), C.byref(coph), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(merge, height, clusters, coph.value))
    if st.value == 0:
        r.update(merge=merge, height=height, clusters=clusters, cophenetic=coph.value)
    return r


# ----------------------------------------------------------------------------- label-guided refinement (ops_refine.hip)
def _opt_ptr(a):
    return _np_ptr(a) if a is not None else None


def _labels_arg(labels):
    return None if labels is None else np.ascontiguousarray(labels, np.int32).reshape(-1)


def compute_target_double(H, labels, n_classes, whiten=True, *, k=None, n=None, init=-7.0):
    """rcppml_gpu_compute_target_double: dict(status, error, target (n, k) row-major = k x n, shift (n_classes, k), counts, buffers).
    H: (n, k) row-major (= k x n column-major) or None (a null pointer); labels: n ints, negative = NA, or None.  Outputs start at
    `init` / -7 (a refused call leaves them so)."""
    Hc = None if H is None else np.ascontiguousarray(H, np.float64)
    lab = _labels_arg(labels)
    if n is None:
        n = Hc.shape[0]
    if k is None:
        k = Hc.shape[1]
    nn, kk, cc = max(int(n), 1), max(int(k), 1), max(int(n_classes), 1)
    T = np.full((nn, kk), init)
    shift = np.full((cc, kk), init)
    counts = np.full(cc, -7, np.int32)
    st = C.c_int(-99)
    lib().rcppml_gpu_compute_target_double(_opt_ptr(Hc), _opt_ptr(lab), _ci(k), _ci(n), _ci(n_classes), _ci(bool(whiten)), _np_ptr(T),
                                           _np_ptr(shift), _np_ptr(counts), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(T, shift, counts))
    if st.value == 0:
        r.update(target=T, shift=shift[:int(n_classes)], counts=counts[:int(n_classes)])
    return r


def refine_correct_double(H, labels, n_classes, lambda_, nonneg=True, whiten=True, *, k=None, n=None, want_target=True, init=-7.0):
    """rcppml_gpu_refine_correct_double (stage 1 of refine()): dict(status, error, H_corr (n, k), target (n, k) or None, buffers)."""
    Hc = None if H is None else np.ascontiguousarray(H, np.float64)
    lab = _labels_arg(labels)
    if n is None:
        n = Hc.shape[0]
    if k is None:
        k = Hc.shape[1]
    nn, kk = max(int(n), 1), max(int(k), 1)
    out = np.full((nn, kk), init)
    T = np.full((nn, kk), init) if want_target else None
    st = C.c_int(-99)
    lib().rcppml_gpu_refine_correct_double(_opt_ptr(Hc), _opt_ptr(lab), _ci(k), _ci(n), _ci(n_classes), _ci(bool(whiten)),
                                           _cd(lambda_), _ci(bool(nonneg)), _np_ptr(out), _opt_ptr(T), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(out,) if T is None else (out, T))
    if st.value == 0:
        r.update(H_corr=out, target=T)
    return r


def refine_wfit_double(csc, dense, m, n, k, d, H_corr, nonneg=True, init=-7.0):
    """rcppml_gpu_refine_wfit_double: dict(status, error, W ((m, k) row-major = k x m), buffers).  csc / dense as in
    score_test_double; d: (k); H_corr: (n, k) row-major."""
    head, keep = _matrix_head(csc, dense)
    dd = None if d is None else np.ascontiguousarray(d, np.float64)
    Hc = None if H_corr is None else np.ascontiguousarray(H_corr, np.float64)
    W = np.full((max(int(m), 1), max(int(k), 1)), init)
    st = C.c_int(-99)
    lib().rcppml_gpu_refine_wfit_double(*head, _ci(m), _ci(n), _ci(k), _opt_ptr(dd), _opt_ptr(Hc), _ci(bool(nonneg)), _np_ptr(W),
                                        C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(W,))
    if st.value == 0:
        r.update(W=W)
    return r


def refine_double(csc, dense, m, n, k, W_T, d, H, labels, n_classes, lambda_=0.8, cycles=0, nonneg=True, whiten=True, init=-7.0):
    """rcppml_gpu_refine_double: dict(status, error, W (m, k), d (k), H (n, k), H_corr (n, k), buffers).  W_T: (m, k) row-major
    (= k x m), H: (n, k) row-major (= k x n); any of them None hands over a null pointer."""
    head, keep = _matrix_head(csc, dense)
    Wc = None if W_T is None else np.ascontiguousarray(W_T, np.float64)
    dd = None if d is None else np.ascontiguousarray(d, np.float64)
    Hc = None if H is None else np.ascontiguousarray(H, np.float64)
    lab = _labels_arg(labels)
    mm, nn, kk = max(int(m), 1), max(int(n), 1), max(int(k), 1)
    oW, od, oH, oC = np.full((mm, kk), init), np.full(kk, init), np.full((nn, kk), init), np.full((nn, kk), init)
    st = C.c_int(-99)
    lib().rcppml_gpu_refine_double(*head, _ci(m), _ci(n), _ci(k), _opt_ptr(Wc), _opt_ptr(dd), _opt_ptr(Hc), _opt_ptr(lab),
                                   _ci(n_classes), _cd(lambda_), _ci(cycles), _ci(bool(nonneg)), _ci(bool(whiten)), _np_ptr(oW),
                                   _np_ptr(od), _np_ptr(oH), _np_ptr(oC), C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(oW, od, oH, oC))
    if st.value == 0:
        r.update(W=oW, d=od, H=oH, H_corr=oC)
    return r


# ----------------------------------------------------------------------------- zero-inflated GP / NB (ops_zi.hip)
ZI_MODE = {"row": 1, "col": 2, "twoway": 3}


def zi_em_double(csc, m, n, k, W_T, d, H, disp, pi, loss_type, zi_mode, zi_em_iters=1, theta_min=0.0, want_imputed=True, init=-7.0):
    """rcppml_gpu_zi_em_double (the E / M / impute stage alone): dict(status, error, pi, disp, imputed (m, n), buffers).  csc: an object
    with p / i / x or a (p, i, x) tuple; W_T (m, k), H (n, k) row-major; disp (m), pi (m for ROW, n for COL) are copied, not changed.
    A refused call leaves the copies as they were handed over and the imputed buffer at `init`."""
    head, keep = _matrix_head(csc, None)
    W_T = np.ascontiguousarray(W_T, np.float64); d = np.ascontiguousarray(d, np.float64); H = np.ascontiguousarray(H, np.float64)
    disp = np.array(disp, np.float64).reshape(-1).copy()
    pi = np.array(pi, np.float64).reshape(-1).copy()
    imp = np.full(max(m * n, 1), init) if want_imputed else None
    st = C.c_int(-99)
    lib().rcppml_gpu_zi_em_double(*head[:4], _ci(m), _ci(n), _ci(k), _np_ptr(W_T), _np_ptr(d), _np_ptr(H), _np_ptr(disp), _ci(loss_type),
                                  _ci(zi_mode), _ci(zi_em_iters), _cd(theta_min), _np_ptr(pi), _opt_ptr(imp), C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(pi, disp, imp), pi=pi, disp=disp)
    if st.value == 0 and imp is not None:
        r["imputed"] = imp[:m * n].reshape(n, m).T.copy()          # column-major m x n
    return r


def nmf_zi_double(p, i, x, m, n, k, W_T, H, *, zi_mode, zi_em_iters=1, loss_type=5, max_iter=100, tol=1e-4, L1_H=0.0, L1_W=0.0,
                  L2_H=0.0, L2_W=0.0, ub_H=0.0, ub_W=0.0, cd_maxit=100, cd_tol=1e-8, verbose=0, patience=5, nonneg_W=1, nonneg_H=1,
                  irls_max_iter=5, irls_tol=1e-4, norm_type=0, dispersion_mode=2, gp_theta=(0.1, 5.0, 0.0), nb_size=(10.0, 1e6, 0.01),
                  sort_model=1, want_history=True, init=-7.0):
    """rcppml_gpu_nmf_zi_double.  W_T (m, k) and H (n, k) float64 (memory = column-major k x m / k x n) are updated IN PLACE.  Returns
    dict(status, error, d, iter, converged, loss, tol, theta, pi, loss_history, buffers); the output buffers start at `init` (d: ones) and a
    refused call leaves them and W_T / H so."""
    p, i, x = _csc_args(p, i, x)
    assert W_T.dtype == np.float64 and H.dtype == np.float64 and W_T.flags.c_contiguous and H.flags.c_contiguous
    assert W_T.shape == (m, k) and H.shape == (n, k)
    d = np.ones(max(k, 1), np.float64)
    theta = np.full(max(m, 1), init)
    pi = np.full(max(m, n, 1), init)
    hist = np.full(max(max_iter, 1), np.nan) if want_history else None
    theta_len, pi_len, out_iter, out_conv, st = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-99)
    out_loss, out_tol = C.c_double(init), C.c_double(init)
    lib().rcppml_gpu_nmf_zi_double(
        _np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(m), _ci(n), _ci(x.shape[0]), _ci(k), _np_ptr(W_T), _np_ptr(H), _np_ptr(d), _ci(max_iter),
        _cd(tol), _cd(L1_H), _cd(L1_W), _cd(L2_H), _cd(L2_W), _cd(ub_H), _cd(ub_W), _ci(cd_maxit), _cd(cd_tol), _ci(verbose), _ci(patience),
        _ci(nonneg_W), _ci(nonneg_H), _ci(loss_type), _ci(irls_max_iter), _cd(irls_tol), _ci(norm_type), _ci(dispersion_mode),
        _cd(gp_theta[0]), _cd(gp_theta[1]), _cd(gp_theta[2]), _cd(nb_size[0]), _cd(nb_size[1]), _cd(nb_size[2]), _ci(sort_model),
        _ci(zi_mode), _ci(zi_em_iters), _np_ptr(hist) if hist is not None else None, _np_ptr(theta), C.byref(theta_len), _np_ptr(pi),
        C.byref(pi_len), C.byref(out_iter), C.byref(out_conv), C.byref(out_loss), C.byref(out_tol), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", d=d[:k], buffers=(d, theta, pi, theta_len.value, pi_len.value,
                                                                                          out_iter.value, out_loss.value))
    if st.value == 0:
        r.update(iter=out_iter.value, converged=bool(out_conv.value), loss=out_loss.value, tol=out_tol.value,
                 theta=theta[:theta_len.value].copy(), pi=pi[:pi_len.value].copy(),
                 loss_history=hist[:out_iter.value].copy() if hist is not None else None)
    return r


# ----------------------------------------------------------------------------- factor graphs (ops_graph.hip)
GRAPH_SRC = {"input": 0, "layer": 1, "concat": 2, "add": 3}


def factor_net_dims(m, n, rank, src_kind, branches, cond_p):
    """(rows_i, cols_i) of every layer's effective input, as rcppml_gpu_factor_net_fit_ex derives them."""
    dims = []
    for i, kind in enumerate(src_kind):
        if kind == 0:
            dims.append((int(m), int(n)))
            continue
        br = list(branches[i])
        rows = dims[br[0]][1]
        cols = (int(rank[br[0]]) if kind == 3 else sum(int(rank[b]) for b in br)) + int(cond_p[i])
        dims.append((rows, cols))
    return dims


def factor_net_fit(csc, dense, m, n, rank, src_kind, branches, cond_Z, L1, L2, upper_bound, nonneg, *, max_iter=100, tol=1e-4, seed=0,
                   solver_mode=1, norm_type=0, cd_maxit=100, cd_tol=1e-8, states=None, init=-7.0):
    """rcppml_gpu_factor_net_fit_ex.  csc / dense as in score_test_double.  rank, src_kind (GRAPH_SRC codes): one per layer; branches:
    per layer the list of upstream layer indices; cond_Z: per layer None or the condition block, p x rows_i; L1, L2, upper_bound,
    nonneg: per layer a (W, H) pair.  states: None (the warm-up runs) or per layer (W (rows_i, k), d (k), H (k, cols_i)) -- the
    warm-up is skipped.  Returns dict(status, error, layers = [(W, d, H)] in the same shapes, layer_loss, iter, converged, loss,
    counts = (device-op calls, own launches) of one outer iteration, buffers).  Without states the packed buffers start at `init`
    and a refused call leaves them so."""
    head, keep = _matrix_head(csc, dense)
    NL = len(rank)
    rk = np.ascontiguousarray(rank, np.int32)
    kind = np.ascontiguousarray(src_kind, np.int32)
    bptr = np.zeros(NL + 1, np.int32)
    for i in range(NL):
        bptr[i + 1] = bptr[i] + len(branches[i])
    bidx = np.ascontiguousarray([b for br in branches for b in br] or [0], np.int32)
    Zs = [None if z is None else np.asarray(z, np.float64) for z in cond_Z]
    cp = np.ascontiguousarray([0 if z is None else z.shape[0] for z in Zs], np.int32)
    zflat = [np.ascontiguousarray(z.T).reshape(-1) for z in Zs if z is not None]
    zbuf = np.concatenate(zflat) if zflat else None
    pen = [np.ascontiguousarray(np.asarray(v, np.float64).reshape(NL, 2)).reshape(-1) for v in (L1, L2, upper_bound)]
    nn = np.ascontiguousarray(np.asarray(nonneg).reshape(NL, 2).astype(np.int32)).reshape(-1)
    try:
        dims = factor_net_dims(m, n, rk, kind, branches, cp)
    except (IndexError, TypeError):
        dims = [(1, 1)] * NL                    # a malformed graph: the entry refuses it before it reads a factor
    nW = sum(max(r, 1) * int(k) for (r, _), k in zip(dims, rk))
    nH = sum(max(c, 1) * int(k) for (_, c), k in zip(dims, rk))
    nd = int(rk.sum())
    if states is not None:
        W = np.concatenate([np.ascontiguousarray(s[0], np.float64).reshape(-1) for s in states])
        d = np.concatenate([np.ascontiguousarray(s[1], np.float64).reshape(-1) for s in states])
        H = np.concatenate([np.ascontiguousarray(np.asarray(s[2], np.float64).T).reshape(-1) for s in states])
    else:
        W, d, H = np.full(max(nW, 1), init), np.full(max(nd, 1), init), np.full(max(nH, 1), init)
    ll = np.full(max(NL, 1), init)
    counts = np.full(2, -7, np.int32)
    it, conv, st = C.c_int(-7), C.c_int(-7), C.c_int(-99)
    loss = C.c_double(init)
    lib().rcppml_gpu_factor_net_fit_ex(*head, _ci(m), _ci(n), _ci(NL), _np_ptr(rk), _np_ptr(kind), _np_ptr(bptr), _np_ptr(bidx), _np_ptr(cp),
                                       _opt_ptr(zbuf), _np_ptr(pen[0]), _np_ptr(pen[1]), _np_ptr(pen[2]), _np_ptr(nn), _ci(max_iter),
                                       _cd(tol), _ci(seed), _ci(solver_mode), _ci(norm_type), _ci(cd_maxit), _cd(cd_tol),
                                       _ci(0 if states is None else 1), _np_ptr(W), _np_ptr(d), _np_ptr(H), _np_ptr(ll), C.byref(it),
                                       C.byref(conv), C.byref(loss), _np_ptr(counts), C.byref(st))
    del keep
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(W, d, H, ll, it.value, conv.value, loss.value))
    if st.value == 0:
        layers, oW, od, oH = [], 0, 0, 0
        for (rows, cols), k in zip(dims, rk):
            k = int(k)
            layers.append((W[oW:oW + rows * k].reshape(rows, k).copy(), d[od:od + k].copy(), H[oH:oH + cols * k].reshape(cols, k).T.copy()))
            oW, od, oH = oW + rows * k, od + k, oH + cols * k
        r.update(layers=layers, layer_loss=ll[:NL].copy(), iter=it.value, converged=bool(conv.value), loss=loss.value,
                 counts=(int(counts[0]), int(counts[1])))
    return r


# ----------------------------------------------------------------------------- column similarities and matching (ops_similarity.hip)
SIMILARITY_METHOD = {"cosine": 0, "cor": 1}


def cosine_geometry():
    """rcppml_gpu_cosine_geometry: dict(tile (columns of x per LDS tile), waves (wavefronts per workgroup), groups (workgroups of the
    default launch before the cap by the work; 0 without a device))."""
    out = (C.c_int64 * 3)()
    f = lib().rcppml_gpu_cosine_geometry
    f.restype = C.c_int
    _chk(f(out), "cosine_geometry")
    return dict(tile=int(out[0]), waves=int(out[1]), groups=int(out[2]))


def _csc_ptrs(a):
    """(col_ptr, row_idx, values, nnz) pointers of a CSC-like object with p / i / x, and the arrays to keep alive."""
    p, i, x = np.ascontiguousarray(a.p, np.int32), np.ascontiguousarray(a.i, np.int32), np.ascontiguousarray(a.x, np.float64)
    return [_np_ptr(p), _np_ptr(i), _np_ptr(x), _ci(x.shape[0])], (p, i, x)


def cosine_sparse(x, y=None, *, m=None, nx=None, ny=None, groups=0, init=-7.0, out=None):
    """rcppml_gpu_cosine_sparse_ex.  x, y: objects with p / i / x and shape (data.CSC), y None for y = x.  m, nx, ny override the
    shapes (tests of the refusals).  out: the result buffer (nx x ny, Fortran order; default a new one filled with `init`).  Returns
    dict(status, error, C (nx x ny), launches, device_ms, download_ms, buffers); a refused call leaves `out` as it was."""
    m = x.shape[0] if m is None else m
    nx = x.shape[1] if nx is None else nx
    ny = (nx if y is None else y.shape[1]) if ny is None else ny
    hx, keep_x = _csc_ptrs(x)
    hy, keep_y = _csc_ptrs(y) if y is not None else ([None, None, None, None], ())
    if out is None:
        out = np.full((max(int(nx), 1), max(int(ny), 1)), init, order="F")
    launches, st = C.c_int(0), C.c_int(-99)
    ms = (C.c_double * 2)(0.0, 0.0)
    lib().rcppml_gpu_cosine_sparse_ex(*hx, *hy, _ci(m), _ci(nx), _ci(ny), _ci(groups), _np_ptr(out), C.byref(launches), ms,
                                      C.byref(st))
    del keep_x, keep_y
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(out,))
    if st.value == 0:
        r.update(C=out, launches=launches.value, device_ms=ms[0], download_ms=ms[1])
    return r


def cosine_dense(W, R, method="cosine", *, m=None, kx=None, ky=None, reps=None, init=-7.0):
    """rcppml_gpu_cosine_dense_ex.  W: (reps, kx, m) C-contiguous (each replicate m x kx column-major), R: (ky, m) C-contiguous
    (m x ky column-major).  method: "cosine" / "cor" or the raw code.  Returns dict(status, error, sim (reps, kx, ky), launches,
    buffers); out[q][a, b] = similarity of column a of W_q and column b of R."""
    W = np.ascontiguousarray(W, np.float64)
    R = np.ascontiguousarray(R, np.float64)
    reps = W.shape[0] if reps is None else reps
    kx = W.shape[1] if kx is None else kx
    m = W.shape[2] if m is None else m
    ky = R.shape[0] if ky is None else ky
    out = np.full((max(int(reps), 1), max(int(ky), 1), max(int(kx), 1)), init)       # each replicate kx x ky column-major
    launches, st = C.c_int(0), C.c_int(-99)
    lib().rcppml_gpu_cosine_dense_ex(_np_ptr(W), _np_ptr(R), _ci(m), _ci(kx), _ci(ky), _ci(reps), _ci(SIMILARITY_METHOD.get(method, method)),
                                     _np_ptr(out), C.byref(launches), C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(out,))
    if st.value == 0:
        r.update(sim=np.ascontiguousarray(out.transpose(0, 2, 1)), launches=launches.value)
    return r


def bipartite_match(cost, *, nr=None, nc=None, batch=None, init=-7):
    """rcppml_gpu_bipartite_match_ex (host only, no device).  cost: (nr, nc) or (batch, nr, nc), or None (a null pointer).  Returns
    dict(status, error, assignment ((batch,) nr ints, -1 for an unmatched row), cost ((batch,) doubles), buffers)."""
    cm = None if cost is None else np.ascontiguousarray(cost, np.float64)
    single = cm is not None and cm.ndim == 2
    if cm is not None:
        c3 = cm[None] if single else cm
        batch = c3.shape[0] if batch is None else batch
        nr = c3.shape[1] if nr is None else nr
        nc = c3.shape[2] if nc is None else nc
    asg = np.full((max(int(batch), 1), max(int(nr), 1)), int(init), np.int32)
    tot = np.full(max(int(batch), 1), float(init))
    st = C.c_int(-99)
    lib().rcppml_gpu_bipartite_match_ex(_np_ptr(cm) if cm is not None else None, _ci(nr), _ci(nc), _ci(batch), _np_ptr(asg), _np_ptr(tot),
                                        C.byref(st))
    r = dict(status=st.value, error=last_error() if st.value else "", buffers=(asg, tot))
    if st.value == 0:
        r.update(assignment=asg[0] if single else asg, cost=float(tot[0]) if single else tot)
    return r
