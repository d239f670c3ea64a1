"""svd() and pca(): host-side mirror of the reference R surface (R/svd.R) on the HIP SVD path (csrc/ops_svd.hip).  Method
resolution, per-method maxit defaults and the validation messages are R's (R/svd.R:118-406) for the arguments this surface takes;
the GPU runs deflation (method "deflation"), Golub-Kahan-Lanczos (every other method, unconstrained), for an explicit
method "krylov" with element constraints the block refinement KSPR of rcppml_gpu_svd_krylov_ex (_abi.svd_krylov), or for an
explicit method "randomized" the randomized block method of rcppml_gpu_svd_randomized_ex (_abi.svd_randomized).  Cross-validation,
auto-rank (k = "auto") and a mask matrix run the deflation of the build-defined rcppml_gpu_svd_cv_ex entries (_abi.svd_cv);
L21, angular and graph regularisation run the same deflation through rcppml_gpu_svd_reg_ex (_abi.svd_reg), with or without CV or a
mask; everything else stays on the reference-shaped entries (_abi.svd_pca).  No CPU fallback: without a device the calls raise
BackendError."""
import numpy as np

from . import _abi
from .data import as_matrix

VALID_METHODS = ("auto", "deflation", "krylov", "lanczos", "irlba", "randomized")
_MISSING = object()


def _gram_level(angular, graph, graph_lambda):
    """R/svd.R:290-292: angular > 0 on a side, or a graph given on a side whose graph_lambda is > 0.  graph: (U given, V given)."""
    ang, lam = np.resize(np.asarray(angular, float), 2), np.resize(np.asarray(graph_lambda, float), 2)
    gr = np.resize(np.asarray(graph, bool), 2)
    return bool(np.any(ang > 0) or (gr[0] and lam[0] > 0) or (gr[1] and lam[1] > 0))


def resolve_method(k, method="auto", maxit=_MISSING, tol=1e-5, L1=0, L2=0, nonneg=False, upper_bound=0, use_gpu=True, *, L21=0,
                   angular=0, graph_lambda=0, graph=(False, False)):
    """R/svd.R:140-406 for the arguments svd() takes here: returns (method, maxit, tol, (L1, L2, nonneg, upper_bound)) or raises
    ValueError with R's message.  graph: which of graph_U / graph_V is given.  L21 counts as an element constraint, angular and an
    active graph as Gram-level constraints (:286-311)."""
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
    L21 = np.resize(np.asarray(L21, float), 2)
    if np.any(L21 < 0):
        raise ValueError("L21 penalties must be non-negative")
    if np.any(np.resize(np.asarray(angular, float), 2) < 0):
        raise ValueError("angular penalties must be non-negative")
    if np.any(np.resize(np.asarray(graph_lambda, float), 2) < 0):
        raise ValueError("graph_lambda must be non-negative")
    if tol < 0:
        raise ValueError("'tol' must be non-negative")
    if not (method in ("lanczos", "irlba", "krylov") and maxit == 0) and maxit < 1:
        raise ValueError("'maxit' must be >= 1")
    constrained = bool(np.any(L1 > 0) or np.any(L2 > 0) or np.any(nonneg) or np.any(upper_bound > 0) or np.any(L21 > 0))
    gram = _gram_level(angular, graph, graph_lambda)
    if method != "auto" and constrained and method not in ("deflation", "krylov"):
        raise ValueError("method '%s' does not support constraints (L1/L2/nonneg/bounds/L21). Use 'deflation' or 'krylov'." % method)
    if method != "auto" and gram and method not in ("deflation", "krylov"):
        raise ValueError("method '%s' does not support Gram-level regularization (angular/graph). Use 'krylov'." % method)
    if method == "auto":
        if constrained or gram:
            method = "krylov" if k >= 8 else "deflation"
        elif use_gpu:
            method = "lanczos" if k < 32 else ("randomized" if k < 64 else "irlba")
        if maxit_missing:
            if method in ("lanczos", "irlba", "krylov"):
                maxit = 0
            elif method == "randomized":
                maxit = 3
    return method, int(maxit), float(tol), (L1, L2, nonneg, upper_bound)


def resolve_mask(mask, shape):
    """R/svd.R:233-269: mask is None, "zeros", a sparse matrix or ("zeros", matrix).  Returns (mask_zeros, (p, i, rows, cols) or
    None) -- the pattern of the mask's nonzero entries, rows ascending -- or raises ValueError with R's message."""
    import scipy.sparse as sp
    mask_zeros, mat = False, None
    if mask is None:
        return False, None
    if isinstance(mask, (list, tuple)):
        if len(mask) < 2 or not isinstance(mask[0], str) or mask[0] != "zeros":
            raise ValueError("'mask' list must be list(\"zeros\", <matrix>)")
        mask_zeros, mat = True, mask[1]
    elif isinstance(mask, str):
        if mask != "zeros":
            raise ValueError("'mask' string must be \"zeros\". Got: '%s'" % mask)
        mask_zeros = True
    else:
        mat = mask
    if mat is None:
        return mask_zeros, None
    if not sp.issparse(mat):
        raise ValueError("'mask' must be NULL, 'zeros', a dgCMatrix, or list(\"zeros\", <dgCMatrix>)")
    mat = sp.csc_matrix(mat)
    mat.eliminate_zeros()
    mat.sum_duplicates()
    mat.sort_indices()
    if mat.shape != tuple(shape):
        raise ValueError("'mask' dimensions (%d x %d) must match 'A' (%d x %d)" % (mat.shape[0], mat.shape[1], shape[0], shape[1]))
    return mask_zeros, (mat.indptr.astype(np.int32), mat.indices.astype(np.int32), mat.shape[0], mat.shape[1])


def resolve_graph(g, lam, dim, name, of):
    """R/svd.R:326-339 for one side: None, or (p, i, x, dim, lambda) of the sparse matrix as given (duplicates summed, rows
    ascending).  Raises ValueError with R's message."""
    import scipy.sparse as sp
    if g is None:
        return None
    if not sp.issparse(g):
        raise ValueError("%s must be a sparse matrix" % name)
    if g.shape != (dim, dim):
        raise ValueError("%s must be %d x %d (matching %s of A)" % (name, dim, dim, of))
    g = sp.csc_matrix(g, dtype=np.float64)
    g.sum_duplicates()
    g.sort_indices()
    return (g.indptr.astype(np.int32), g.indices.astype(np.int32), g.data.astype(np.float64), dim, float(lam))


def resolve_cv(k, method="auto", test_fraction=0, patience=3, k_max=50, L1=0, L2=0, nonneg=False, upper_bound=0, *, L21=0, angular=0,
               graph_lambda=0, graph=(False, False)):
    """The cross-validation rules of R/svd.R beside resolve_method(): :177-186 (k = "auto" sets k = k_max and test_fraction = 0.05
    when it is <= 0), :216-217 (ranges), :313-321 (a method without CV raises under auto-rank and drops CV silently under a fixed
    k), :377-385 (method "auto" under CV is deflation, or krylov for a constrained k >= 8).  Returns (k, method, test_fraction,
    auto_rank); the method goes through resolve_method() afterwards."""
    auto_rank = isinstance(k, str) and k == "auto"
    if auto_rank:
        k = int(k_max)
        if test_fraction <= 0:
            test_fraction = 0.05
    else:
        k = int(k)
        if k < 1:
            raise ValueError("'k' must be >= 1")
    if test_fraction < 0 or test_fraction >= 1:
        raise ValueError("'test_fraction' must be in [0, 1)")
    if patience < 1:
        raise ValueError("'patience' must be >= 1")
    has_cv = auto_rank or 0 < test_fraction < 1
    if method not in VALID_METHODS:
        raise ValueError("method must be one of: %s" % ", ".join(VALID_METHODS))
    constrained = any(bool(np.any(np.asarray(v, float) > 0)) for v in (L1, L2, nonneg, upper_bound, L21))
    constrained = constrained or _gram_level(angular, graph, graph_lambda)
    if method == "auto":
        if has_cv:
            method = "krylov" if constrained and k >= 8 else "deflation"
    elif has_cv and method not in ("deflation", "krylov") and not constrained:   # constrained: resolve_method() raises first, as R
        if auto_rank:
            raise ValueError("method '%s' does not support auto-rank. Use 'deflation' or 'krylov'." % method)
        test_fraction = 0
    return k, method, float(test_fraction), auto_rank


def svd(A, k=10, tol=1e-5, maxit=_MISSING, center=False, seed=None, L1=0, L2=0, nonneg=False, upper_bound=0, method="auto",
        precision="float", test_fraction=0, mask=None, cv_seed=None, patience=3, k_max=50, L21=0, angular=0, graph_U=None,
        graph_V=None, graph_lambda=0):
    """Truncated SVD on the GPU (R/svd.R with resource = "gpu").  A: scipy sparse / CSC (the sparse entries) or a dense matrix (the
    dense entries).  precision: "float" (fp32 on the device, R's default) or "double".

    method="krylov" with L1, L2, nonneg or upper_bound runs Krylov-Seeded Projected Refinement: a Lanczos seed, then passes of
    Gram-solve-and-project on all k factors at once (k <= 128); maxit is the pass limit (missing: max(10, 2 ceil(log2 k) + 3), as R
    resolves krylov's maxit to 0) and tol the bound on the relative change of u that ends the passes.  With nonneg, L1 or an upper
    bound the factors come back as they are, ordered by d; with L2 only they are re-orthogonalised.  Without constraints krylov is
    Lanczos.  method="auto" still resolves constrained fits with k >= 8 to krylov as in R, and that resolution is still refused
    (BackendError): name method="krylov" or method="deflation" for them.

    method="randomized", named, runs the randomized block method (Halko-Martinsson-Tropp, the reference's svd/randomized.hpp): a
    sketch of l = k + max(10, k / 5) <= 128 columns, maxit power iterations (missing: 3, at most 10; tol is not used) and a small
    SVD of the projected matrix -- a fixed cost, iters_per_factor = [the power iterations run].  Its answer is an approximation of the truncated SVD,
    good where the spectrum decays: at k = 40 with 3 power iterations the tail singular values of the movielens fixture come out 4 %
    below the true ones and those of hawaiibirds 1 % below (the leading ones agree far better).  It takes no constraint,
    cross-validation or mask.  method="auto" keeps running Lanczos where R resolves it to randomized (32 <= k < 64).

    k = "auto" (rank up to k_max, default 50) or test_fraction > 0 holds out a speckled set of entries and stops adding factors
    when their error has not improved for `patience` factors, with a fixed k too, so fewer than k factors may come back; the
    result is trimmed to the best rank.  mask: None, "zeros" (only stored entries are held out), a sparse matrix whose nonzero
    entries are unobserved, or ("zeros", matrix).  cv_seed: seed of the hold-out set (None: derived from seed).  These run
    deflation; under CV or a mask matrix krylov is refused on the GPU, and so is a mask matrix with any method but deflation.  A rank above
    min(m, n) is clamped here (the reference's gateway passes k_max on unchanged and its loop then ends on sigma ~ 0).

    L21, angular (one value or one per side, u then v) and graph_U (m x m) / graph_V (n x n) with graph_lambda (one value or one per
    side) are R's three further regularisers, applied in every deflation iteration after the element constraints: L21 adds
    L21 / |x| to L2, angular pulls the update away from the factors already stored, and a graph takes the gradient step
    x -= (graph_lambda / nsq) L x -- keep graph_lambda * lambda_max(L) well below the squared norm it is divided by, or the step
    amplifies instead of smoothing.  They run with method "deflation", with or without CV or a mask; method "krylov" with any of
    them on, named or reached through "auto" (k >= 8), is refused on the GPU: pass method = "deflation".

    Returns dict(u, d, v, misc) with misc = dict(iters_per_factor, frobenius_norm_sq, row_means (or None), method, wall_time_ms,
    auto_rank, k_selected, test_loss (one value per computed factor; empty without CV), n_test, cv_seed_effective); under KSPR
    also passes and dw (the relative change of u in each pass from the second on), and iters_per_factor is empty."""
    explicit = method
    M, dense = as_matrix(A, what="'A' must be a matrix, dgCMatrix, or path to a .spz file")
    shape = dense.shape if dense is not None else (M.rows, M.cols)
    new = dict(L21=L21, angular=angular, graph_lambda=graph_lambda, graph=(graph_U is not None, graph_V is not None))
    k, method, test_fraction, auto_rank = resolve_cv(k, method, test_fraction, patience, k_max, L1, L2, nonneg, upper_bound, **new)
    method, maxit, tol, (L1v, L2v, nn, ub) = resolve_method(k, method, maxit, tol, L1, L2, nonneg, upper_bound, **new)
    mask_zeros, obs = resolve_mask(mask, shape)
    L21v, angv, lam = (np.resize(np.asarray(v, float), 2) for v in (L21, angular, graph_lambda))
    gu = resolve_graph(graph_U, lam[0], shape[0], "graph_U", "rows")
    gv = resolve_graph(graph_V, lam[1], shape[1], "graph_V", "columns")
    if precision not in ("float", "double"):
        raise ValueError("precision must be 'float' or 'double'")
    s = 0 if seed is None else int(seed)
    cs = 0 if cv_seed is None else int(cv_seed)
    if np.any(L21v > 0) or _gram_level(angv, new["graph"], lam):
        if method != "deflation":
            raise _abi.BackendError("GPU SVD/PCA failed: L21, angular and graph regularisation run only in the deflation loop on the GPU "
                                    "(method '%s' has no such terms yet): pass method = \"deflation\"" % method)
        reg = dict(L21=L21v, angular=angv, graph_u=gu if lam[0] > 0 else None, graph_v=gv if lam[1] > 0 else None)
        return _svd_cv(M, dense, min(k, min(shape)), method, maxit, tol, center, s, (L1v, L2v, nn, ub), precision, test_fraction, cs,
                       int(patience), mask_zeros, obs, auto_rank, reg=reg)
    if test_fraction > 0 or obs is not None:
        return _svd_cv(M, dense, min(k, min(shape)), method, maxit, tol, center, s, (L1v, L2v, nn, ub), precision, test_fraction, cs,
                       int(patience), mask_zeros, obs, auto_rank)
    constrained = bool(np.any(L1v > 0) or np.any(L2v > 0) or np.any(nn) or np.any(ub > 0))
    if method == "krylov" and constrained:
        if explicit != "krylov":
            raise _abi.BackendError("GPU SVD/PCA failed: method 'auto' resolves a constrained fit with k >= 8 to 'krylov', which the GPU "
                                    "runs only when it is named: pass method = \"krylov\" (block refinement) or method = \"deflation\"")
        return _svd_krylov(M, dense, min(k, min(shape)), maxit, tol, center, s, (L1v, L2v, nn, ub), precision)
    if explicit == "randomized":
        return _svd_randomized(M, dense, min(k, min(shape)), maxit, center, s, precision)
    kw = dict(precision=precision, tol=tol, max_iter=maxit, center=center, seed=s, L1=L1v, L2=L2v, nonneg=nn, upper_bound=ub,
              algorithm=_abi.SVD_ALGORITHMS[method])
    r = _fitted(_abi.svd_pca, M, dense, int(k), **kw)
    return _packed(r, center, method, r["iters"][:int(np.sum(r["iters"] > 0)) or r["k"]])


def _fitted(call, M, dense, k, **kw):
    """The result of one _abi wrapper on the matrix, or BackendError with the entry's reason."""
    r = call(dense if dense is not None else (M.p, M.i, M.x, M.rows, M.cols), k, dense=dense is not None, **kw)
    if r["status"] != 0:
        raise _abi.BackendError("GPU SVD/PCA failed: %s" % r["error"])
    return r


def _packed(r, center, method, iters, auto_rank=False, test_loss=None, n_test=0, cv_seed_effective=None, **extras):
    """dict(u, d, v, misc) from the result of _fitted(), trimmed to the selected rank.  iters: the iteration counts that count;
    extras: further misc entries (KSPR's)."""
    ks = r["k"]
    misc = dict(iters_per_factor=iters.copy(), frobenius_norm_sq=r["frob"],
                row_means=r["row_means"][:r["U"].shape[0]].copy() if center else None, method=method, wall_time_ms=r["wall_ms"],
                auto_rank=auto_rank, k_selected=ks, test_loss=np.zeros(0) if test_loss is None else test_loss.copy(), n_test=n_test,
                cv_seed_effective=cv_seed_effective, **extras)
    return dict(u=r["U"][:, :ks].copy(), d=r["d"][:ks].copy(), v=r["V"][:, :ks].copy(), misc=misc)


def _svd_cv(M, dense, k, method, maxit, tol, center, seed, cons, precision, test_fraction, cv_seed, patience, mask_zeros, obs, auto_rank,
            reg=None):
    """The cross-validated / masked call: deflation through _abi.svd_cv, or through _abi.svd_reg with reg = its further keywords."""
    if method != "deflation":
        raise _abi.BackendError("GPU SVD/PCA failed: cross-validation, auto-rank and a mask matrix need method 'deflation' on the GPU "
                                "(got '%s')" % method)
    L1v, L2v, nn, ub = cons
    r = _fitted(_abi.svd_cv if reg is None else _abi.svd_reg, M, dense, k, precision=precision, tol=tol, max_iter=maxit,
                center=center, seed=seed, L1=L1v, L2=L2v, nonneg=nn, upper_bound=ub, test_fraction=test_fraction, cv_seed=cv_seed,
                patience=patience, mask_zeros=mask_zeros, obs_mask=obs, **(reg or {}))
    kc = r["k_computed"]
    s32, c32 = seed & 0xFFFFFFFF, cv_seed & 0xFFFFFFFF
    eff = (c32 if c32 != 0 else ((s32 ^ 0xBEEF) if s32 != 0 else 42)) if test_fraction > 0 else None    # core/svd_config.hpp:149-151
    test_loss = r["test_loss"][:kc] if test_fraction > 0 else None
    return _packed(r, center, method, r["iters"][:kc], auto_rank, test_loss, r["n_test"], eff)


def _svd_krylov(M, dense, k, maxit, tol, center, seed, cons, precision):
    """The constrained krylov call: KSPR through _abi.svd_krylov."""
    L1v, L2v, nn, ub = cons
    r = _fitted(_abi.svd_krylov, M, dense, k, precision=precision, tol=tol, max_iter=maxit, center=center, seed=seed, L1=L1v,
                L2=L2v, nonneg=nn, upper_bound=ub)
    return _packed(r, center, "krylov", np.zeros(0, np.int32), passes=r["passes"], dw=r["dw"].copy())


def _svd_randomized(M, dense, k, maxit, center, seed, precision):
    """The named randomized call: the block method through _abi.svd_randomized."""
    r = _fitted(_abi.svd_randomized, M, dense, k, precision=precision, max_iter=maxit, center=center, seed=seed)
    return _packed(r, center, "randomized", r["iters"][:1])


def pca(A, k=10, **kw):
    """svd(A, k, center=True, ...) (R/svd.R:596)."""
    kw["center"] = True
    return svd(A, k=k, **kw)
