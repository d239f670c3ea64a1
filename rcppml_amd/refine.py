"""Label-guided refinement: host-side mirror of the reference's compute_target() (R/compute_target.R) and refine() (R/refine.R)
on the HIP path (csrc/ops_refine.hip).  compute_target() turns class labels into the k x n target that nmf(target_H=...) takes;
refine() shifts an embedding toward its class centroids and, with cycles > 0, propagates the correction through W-refit cycles
that stay on the device.  With `batch` and cycles > 0 the H step of a cycle is the existing target fit of nmf() (PROJ_ADV with the
batch target), driven from here: the W-refit entry, then nmf(maxit=1, precision="fp64"), then the stage-1 correction.  Labels may
be ints, strings or anything sortable; the levels are the sorted unique non-missing values and None / nan / masked entries are
R's NA (the column is left unguided).  No CPU fallback: without a device both functions raise BackendError."""
import numpy as np

from . import _abi
from . import nmf as _nmf
from ._abi import _check
from .data import as_matrix


def _is_na(v):
    if v is None or v is np.ma.masked:
        return True
    try:
        return bool(v != v)          # nan
    except Exception:
        return False


def as_factor(labels):
    """R's as.factor: (codes, levels) with codes int32 in 0 .. len(levels) - 1 and -1 for NA; levels = the sorted unique
    non-missing values."""
    if labels is None:
        return np.zeros(0, np.int32), []
    if isinstance(labels, np.ma.MaskedArray):
        vals = [np.ma.masked if m else v for v, m in zip(labels.data.ravel().tolist(), np.ma.getmaskarray(labels).ravel())]
    else:
        vals = np.asarray(labels, dtype=object).ravel().tolist()
    vals = [v.item() if isinstance(v, np.generic) else v for v in vals]
    levels = sorted(set(v for v in vals if not _is_na(v)))
    index = {v: i for i, v in enumerate(levels)}
    codes = np.array([-1 if _is_na(v) else index[v] for v in vals], np.int32).reshape(-1)
    return codes, levels


def compute_target(H, labels, whiten=True):
    """R's compute_target: the k x n target of a k x n embedding and n class labels.  Each labelled column is its class centroid
    minus the mean of the class centroids (OAS-shrunk ZCA-whitened when `whiten` and there are at least two classes); NA columns are
    zero.  Pass it to nmf(..., target_H=T, target_lambda=0.5) for enrichment or a negative target_lambda for batch removal."""
    if isinstance(H, (str, bytes)) or np.ndim(H) != 2:
        raise ValueError("'H' must be a k x n matrix")
    H = np.asarray(H, np.float64)
    k, n = H.shape
    codes, levels = as_factor(labels)
    if codes.shape[0] != n:
        raise ValueError("length(labels) must equal ncol(H)")
    r = _check(_abi.compute_target_double(H.T, codes, len(levels), whiten), "compute_target")
    return np.ascontiguousarray(r["target"].T)


def _stage1(H, codes, C, lambda_, nonneg, whiten):
    r = _check(_abi.refine_correct_double(H.T, codes, C, lambda_, nonneg, whiten, want_target=False), "refine (correction)")
    return np.ascontiguousarray(r["H_corr"].T)


def _matrix_forms(data, m, n):
    """(csc, dense) for the entries that take either form; a 2-D ndarray is the reference's dense matrix, anything else goes
    sparse."""
    csc, dense = as_matrix(data, dense_ok=isinstance(data, np.ndarray))
    shape = tuple((csc if dense is None else dense).shape)
    if shape != (m, n):
        raise ValueError("dimensions of 'data' (%d x %d) do not match the model (%d x %d)" % (shape + (m, n)))
    return csc, dense


def refine(x, data=None, labels=None, batch=None, lambda_=0.8, cycles=0, nonneg=True, whiten=True):
    """R's refine: post-hoc centroid correction H + lambda * s * T of an nmf model or a k x n matrix (T = compute_target(H, labels),
    s = ||H||_F / ||T||_F, clipped at 0 when `nonneg`), then `cycles` W-refit cycles for a model: W = solve(G + 1e-8 I, B) from the
    corrected H, H from the new W, d = the row norms of H, and the correction again.  `batch` (with cycles > 0): the H step is
    nmf(data, k, seed=W_new, maxit=1, target_H=compute_target(H, batch, whiten=False), target_lambda=(0, -lambda)).  Returns a
    model when x is one (w and d replaced when cycles > 0, h = the corrected H), else the corrected k x n matrix."""
    is_nmf = isinstance(x, _nmf.NMFModel)
    if is_nmf:
        H = np.asarray(x.h, np.float64)
        W = np.asarray(x.w, np.float64)
        d = np.asarray(x.d, np.float64)
    elif isinstance(x, np.ndarray) and x.ndim == 2:
        H = np.asarray(x, np.float64)
        W = d = None
    else:
        raise ValueError("'x' must be an nmf object or a k x n matrix")
    k, n = H.shape
    codes, levels = as_factor(labels)
    if codes.shape[0] != n:
        raise ValueError("length(labels) must equal ncol(H) [= %d]" % n)
    if not (0 <= lambda_ <= 1):
        raise ValueError("'lambda' must be in [0, 1]")
    cycles = int(cycles)
    if cycles > 0 and data is None:
        raise ValueError("'data' is required when cycles > 0")
    has_batch = batch is not None
    if has_batch:
        bcodes, blevels = as_factor(batch)
        if bcodes.shape[0] != n:
            raise ValueError("length(batch) must equal ncol(H) [= %d]" % n)
    C = len(levels)
    lambda_, nonneg, whiten = float(lambda_), bool(nonneg), bool(whiten)
    if not (cycles > 0 and is_nmf):
        H_corr = _stage1(H, codes, C, lambda_, nonneg, whiten)
        return _nmf.NMFModel(w=x.w, d=x.d, h=H_corr, misc=x.misc) if is_nmf else H_corr
    m = W.shape[0]
    csc, dense = _matrix_forms(data, m, n)
    if not has_batch:
        r = _check(_abi.refine_double(csc, dense, m, n, k, W, d, H.T, codes, C, lambda_, cycles, nonneg, whiten), "refine")
        return _nmf.NMFModel(w=r["W"], d=r["d"], h=np.ascontiguousarray(r["H_corr"].T), misc=x.misc)
    # batch removal through the target fit (R/refine.R:129-157); the batch target is computed once, from the original H
    batch_target = np.ascontiguousarray(
        _check(_abi.compute_target_double(H.T, bcodes, len(blevels), False), "compute_target")["target"].T)
    H_corr = _stage1(H, codes, C, lambda_, nonneg, whiten)
    for _ in range(cycles):
        W_new = _check(_abi.refine_wfit_double(csc, dense, m, n, k, d, H_corr.T, nonneg), "refine (W refit)")["W"]
        fit = _nmf.nmf(data, k, seed=W_new, maxit=1, nonneg=nonneg, target_H=batch_target, target_lambda=(0.0, -lambda_),
                       precision="fp64")
        W, d, H = np.asarray(fit.w, np.float64), np.asarray(fit.d, np.float64), np.asarray(fit.h, np.float64)
        H_corr = _stage1(H, codes, C, lambda_, nonneg, whiten)
    return _nmf.NMFModel(w=W, d=d, h=H_corr, misc=x.misc)
