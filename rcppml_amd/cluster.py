"""bipartition() and dclust(): host-side mirror of the reference R surface (R/bipartition.R, R/dclust.R) on the HIP clustering
path (csrc/ops_cluster.hip).  The result is what the reference's CPU path computes (Rcpp_bipartition / Rcpp_dclust_sparse,
src/RcppFunctions_utils.cpp:217-285): sample indices 0-based, as Rcpp returns them.  No CPU fallback: without a device the calls
raise BackendError."""
import numpy as np

from . import _abi
from .data import as_matrix


def _as_csc(data):
    return as_matrix(data, dense_ok=False)[0]      # dense input goes sparse, as R's .to_dgCMatrix (R/dclust.R)


def _seed(seed):
    # R: `if (!is.numeric(seed)) seed <- 0`
    if seed is None:
        return 0.0
    s = float(seed)
    if not (0 <= s < 2 ** 32):
        raise ValueError("'seed' must be in [0, 2^32)")
    return s


def _common(tol, maxit):
    if int(maxit) < 1:
        raise ValueError("'maxit' must be at least 1")
    if not float(tol) < 1:
        raise ValueError("'tol' must be below 1")


def bipartition(data, tol=1e-5, nonneg=True, samples=None, seed=None, calc_dist=True, maxit=100):
    """Spectral bipartition of a sample set by rank-2 NMF (R/bipartition.R).  samples: 0-based column indices (default: all; any
    order, duplicates allowed).  Returns dict(v, dist, size1, size2, samples1, samples2, center1, center2)."""
    A = _as_csc(data)
    _common(tol, maxit)
    if samples is not None:
        samples = np.asarray(samples, dtype=np.int64).ravel()
        if samples.size == 0:
            raise ValueError("'samples' must not be empty")
        if samples.min() < 0:
            raise ValueError("sample indices must be strictly positive")        # R's message, for 1-based indices
        if samples.max() >= A.cols:
            raise ValueError("sample indices must be strictly less than the number of columns in 'data'")
    r = _abi.bipartition_ex(A.p, A.i, A.x, A.rows, A.cols, samples, max_iter=int(maxit), tol=float(tol), nonneg=bool(nonneg),
                            seed=_seed(seed), calc_dist=bool(calc_dist))
    if r["status"] != 0:
        raise _abi.BackendError("GPU bipartition failed: %s" % r["error"])
    smp = np.arange(A.cols) if samples is None else samples
    side1 = r["partition"] == 0
    m = A.rows
    return dict(v=r["v"].copy(), dist=r["dist"], size1=r["size1"], size2=r["size2"], samples1=smp[side1], samples2=smp[~side1],
                center1=r["center"][:m].copy(), center2=r["center"][m:2 * m].copy())


def dclust(A, min_samples, min_dist=0, tol=1e-5, maxit=100, nonneg=True, seed=None):
    """Divisive clustering by recursive bipartition (R/dclust.R).  Returns the clusters in the reference CPU's order: a list of
    dict(samples (0-based), center, id (binary path string), size)."""
    A = _as_csc(A)
    _common(tol, maxit)
    if int(min_samples) < 1:
        raise ValueError("'min_samples' must be at least 1")
    r = _abi.dclust_ex(A.p, A.i, A.x, A.rows, A.cols, min_samples=int(min_samples), min_dist=float(min_dist), max_iter=int(maxit),
                       tol=float(tol), nonneg=bool(nonneg), seed=_seed(seed))
    if r["status"] != 0:
        raise _abi.BackendError("GPU dclust failed: %s" % r["error"])
    asg = r["assignments"]
    order = np.argsort(asg, kind="stable")
    bounds = np.searchsorted(asg[order], np.arange(r["clusters"] + 1))
    return [dict(samples=order[bounds[c]:bounds[c + 1]], center=r["center"][c].copy(), id=r["ids"][c], size=int(r["size"][c]))
            for c in range(r["clusters"])]
