"""svd() and pca(): host-side mirror of the reference R surface (R/svd.R) on the HIP SVD path (csrc/ops_svd.hip).  Method
resolution, per-method maxit defaults and the validation messages are R's (R/svd.R:118-406) for the arguments this surface takes;
the GPU runs deflation (method "deflation") or Golub-Kahan-Lanczos (every other method, unconstrained).  No CPU fallback: without
a device the calls raise BackendError."""
import numpy as np

from . import _abi
from .data import as_matrix

VALID_METHODS = ("auto", "deflation", "krylov", "lanczos", "irlba", "randomized")
_MISSING = object()


def resolve_method(k, method="auto", maxit=_MISSING, tol=1e-5, L1=0, L2=0, nonneg=False, upper_bound=0, use_gpu=True):
    """R/svd.R:140-406 for the arguments svd() takes here: returns (method, maxit, tol) or raises ValueError with R's message."""
    maxit_missing = maxit is _MISSING
    if maxit_missing:
        maxit = 200
    if method != "auto":
        if method in ("lanczos", "irlba", "krylov") and maxit_missing:
            maxit = 0
        if method == "randomized" and maxit_missing:
            maxit = 3
    if method not in VALID_METHODS:
        raise ValueError("method must be one of: %s" % ", ".join(VALID_METHODS))
    k = int(k)
    if k < 1:
        raise ValueError("'k' must be >= 1")
    L1, L2 = np.resize(np.asarray(L1, float), 2), np.resize(np.asarray(L2, float), 2)
    nonneg, upper_bound = np.resize(np.asarray(nonneg, bool), 2), np.resize(np.asarray(upper_bound, float), 2)
    if np.any(L1 < 0):
        raise ValueError("L1 penalties must be non-negative")
    if np.any(L2 < 0):
        raise ValueError("L2 penalties must be non-negative")
    if np.any(upper_bound < 0):
        raise ValueError("upper_bound must be non-negative")
    if tol < 0:
        raise ValueError("'tol' must be non-negative")
    if not (method in ("lanczos", "irlba", "krylov") and maxit == 0) and maxit < 1:
        raise ValueError("'maxit' must be >= 1")
    constrained = bool(np.any(L1 > 0) or np.any(L2 > 0) or np.any(nonneg) or np.any(upper_bound > 0))
    if method != "auto" and constrained and method not in ("deflation", "krylov"):
        raise ValueError("method '%s' does not support constraints (L1/L2/nonneg/bounds/L21). Use 'deflation' or 'krylov'." % method)
    if method == "auto":
        if constrained:
            method = "krylov" if k >= 8 else "deflation"
        elif use_gpu:
            method = "lanczos" if k < 32 else ("randomized" if k < 64 else "irlba")
        if maxit_missing:
            if method in ("lanczos", "irlba", "krylov"):
                maxit = 0
            elif method == "randomized":
                maxit = 3
    return method, int(maxit), float(tol), (L1, L2, nonneg, upper_bound)


def svd(A, k=10, tol=1e-5, maxit=_MISSING, center=False, seed=None, L1=0, L2=0, nonneg=False, upper_bound=0, method="auto",
        precision="float"):
    """Truncated SVD on the GPU (R/svd.R with resource = "gpu").  A: scipy sparse / CSC (the sparse entries) or a dense matrix (the
    dense entries).  precision: "float" (fp32 on the device, R's default) or "double".  Constrained fits with k >= 8 resolve to
    krylov, as in R, which the GPU refuses (BackendError); pass method="deflation" for them.  Returns dict(u, d, v, misc) with
    misc = dict(iters_per_factor, frobenius_norm_sq, row_means (or None), method, wall_time_ms)."""
    M, dense = as_matrix(A, what="'A' must be a matrix, dgCMatrix, or path to a .spz file")
    method, maxit, tol, (L1v, L2v, nn, ub) = resolve_method(k, method, maxit, tol, L1, L2, nonneg, upper_bound)
    if precision not in ("float", "double"):
        raise ValueError("precision must be 'float' or 'double'")
    s = 0 if seed is None else int(seed)
    kw = dict(precision=precision, tol=tol, max_iter=maxit, center=center, seed=s, L1=L1v, L2=L2v, nonneg=nn, upper_bound=ub,
              algorithm=_abi.SVD_ALGORITHMS[method])
    if dense is not None:
        r = _abi.svd_pca(dense, int(k), dense=True, **kw)
        m = dense.shape[0]
    else:
        r = _abi.svd_pca((M.p, M.i, M.x, M.rows, M.cols), int(k), **kw)
        m = M.rows
    if r["status"] != 0:
        raise _abi.BackendError("GPU SVD/PCA failed: %s" % r["error"])
    ks = r["k"]
    iters = r["iters"]
    nz = int(np.sum(iters > 0)) or ks
    misc = dict(iters_per_factor=iters[:nz].copy(), frobenius_norm_sq=r["frob"],
                row_means=r["row_means"][:m].copy() if center else None, method=method, wall_time_ms=r["wall_ms"])
    return dict(u=r["U"][:, :ks].copy(), d=r["d"][:ks].copy(), v=r["V"][:, :ks].copy(), misc=misc)


def pca(A, k=10, **kw):
    """svd(A, k, center=True, ...) (R/svd.R:596)."""
    kw["center"] = True
    return svd(A, k=k, **kw)
