"""cosine(), bipartiteMatch() and align(): host-side mirror of the reference's similarity tools (R/cosine.R, R/bipartiteMatch.R,
R/nmf_methods.R:261-271) on the HIP similarity path (csrc/ops_similarity.hip).  The argument forms, return shapes and messages are
R's; the computation is the three build-defined entries.  cosine() and align() have no CPU fallback: without a device they raise
BackendError.  bipartiteMatch() runs on the host (the entry does no device work).

Rules and deviations from R, all documented in DESIGN.md 4.16:
  * A column of zero norm has cosine 0 to every column, itself included.  R's answer depends on storage: 0 for a column
    that stores nothing (its Inf scale meets no entry), NaN for one that stores explicit zeros (0 * Inf).
  * cosine(vector x, matrix y): R/cosine.R:47 multiplies x by |x|^2 where it should divide by |x|, so it does not return a cosine.
    This build returns the cosine.
  * align(): bipartiteMatch's assignment[i] is the ref factor matched to object factor i.  R/nmf_methods.R:270 indexes the object
    by that vector, which applies the permutation where its inverse is needed (right only when the permutation is its own inverse).
    This build does what the documentation promises: aligned factor j is the object factor matched to ref factor j, that is
    order = argsort(assignment).  misc["assignment"] keeps the raw assignment.
"""
import warnings

import numpy as np

from . import _abi
from .data import CSC, as_matrix
from .nmf import NMFModel

DENSE_MAX_COLUMNS = 128
METHODS = ("cosine", "cor")


def _is_vector(a):
    return not isinstance(a, CSC) and not hasattr(a, "tocsc") and np.ndim(a) == 1


def _as_input(a):
    """(csc, dense, was_vector): a vector becomes an m x 1 dense matrix."""
    if _is_vector(a):
        return None, np.asarray(a, dtype=np.float64).reshape(-1, 1), True
    csc, dense = as_matrix(a, what="x and y must be matrices or vectors")
    return csc, dense, False


def _to_csc(csc, dense):
    """A dense matrix goes sparse with its zeros dropped, as R's .to_dgCMatrix does."""
    return csc if csc is not None else as_matrix(dense, dense_ok=False)[0]


def cosine(x, y=None):
    """Column-by-column cosine similarity (R's cosine).  x, y: numpy 2-D arrays, scipy sparse matrices, CSC, or 1-D vectors.
    matrix x matrix gives (nx, ny), matrix x vector or vector x matrix a vector, vector x vector a scalar; y=None compares the
    columns of x with each other.  Two dense inputs with at most 128 columns each run on the dense entry, everything else on the
    sparse one."""
    if y is None and _is_vector(x):
        raise ValueError("x is a vector and y is NULL")
    xc, xd, xv = _as_input(x)
    yc, yd, yv = _as_input(y) if y is not None else (None, None, False)
    rows_x = (xc if xc is not None else xd).shape[0]
    if y is not None and (yc if yc is not None else yd).shape[0] != rows_x:
        raise ValueError("x and y must have the same number of rows")
    dense_pair = xd is not None and (y is None or yd is not None)
    if dense_pair and xd.shape[1] <= DENSE_MAX_COLUMNS and (y is None or yd.shape[1] <= DENSE_MAX_COLUMNS) and xd.shape[1] >= 1:
        ref = xd if y is None else yd
        r = _abi._check(_abi.cosine_dense(np.ascontiguousarray(xd.T)[None], np.ascontiguousarray(ref.T), "cosine"), "cosine")
        out = r["sim"][0]
    else:
        r = _abi._check(_abi.cosine_sparse(_to_csc(xc, xd), None if y is None else _to_csc(yc, yd)), "cosine")
        out = np.ascontiguousarray(r["C"])
    if xv and yv:
        return float(out[0, 0])
    if xv or yv:
        return out.reshape(-1)
    return out


def bipartiteMatch(x, verbose=False):
    """Minimum-cost bipartite matching of a cost matrix (R's bipartiteMatch): {"cost", "assignment"}, assignment[i] = the column
    matched to row i, 0-indexed as in R (-1 for a row left unmatched when there are more rows than columns).  Negative costs count
    as 0; verbose=True warns about them."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be a matrix")
    if verbose and x.size and x.min() < 0:
        warnings.warn("Negative values in 'x' were replaced by zero. Negative values are not permitted!")
    r = _abi._check(_abi.bipartite_match(x), "bipartiteMatch")
    return {"cost": r["cost"], "assignment": r["assignment"].astype(np.int64)}


def similarity_cost(sim):
    """align()'s cost of a similarity matrix: 1 - sim + 1e-10, negatives set to 0 (R/nmf_methods.R:265-269)."""
    cost = 1.0 - np.asarray(sim, dtype=np.float64) + 1e-10
    cost[cost < 0] = 0.0
    return cost


def align_order(assignment):
    """The factor order that aligns an object to its reference: aligned factor j = the object factor matched to ref factor j."""
    return np.argsort(np.asarray(assignment), kind="stable")


def permute_model(model, order, assignment):
    misc = dict(model.misc) if model.misc else {}
    misc["assignment"] = np.asarray(assignment).copy()
    return NMFModel(model.w[:, order], model.d[order], model.h[order, :], misc)


def align(object, ref, method="cosine"):
    """Reorder the factors of `object` (an NMFModel, or a list of them) to best match `ref` (R's align): bipartite matching on
    1 - cosine (or 1 - correlation, method="cor") of the w matrices.  A list is handled in one device call and one batched match,
    and a list comes back."""
    if method not in METHODS:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in METHODS))
    single = isinstance(object, NMFModel)
    models = [object] if single else list(object)
    if not models:
        return []
    rw = np.asarray(ref.w, dtype=np.float64)
    for mod in models:
        if np.shape(mod.w) != rw.shape:
            raise ValueError("dimensions of object$w and ref$w are not identical")
    if rw.shape[1] > DENSE_MAX_COLUMNS:
        raise ValueError("align() takes models of rank %d at most" % DENSE_MAX_COLUMNS)
    W = np.stack([np.ascontiguousarray(np.asarray(mod.w, dtype=np.float64).T) for mod in models])
    sim = _abi._check(_abi.cosine_dense(W, np.ascontiguousarray(rw.T), method), "align")["sim"]
    assignment = _abi._check(_abi.bipartite_match(similarity_cost(sim)), "align (match)")["assignment"]
    out = [permute_model(mod, align_order(a), a) for mod, a in zip(models, assignment)]
    return out[0] if single else out
