"""numpy/scipy restatement of the reference's CPU bipartition() and dclust() -- the parity target of the GPU clustering path
(rcppml_amd/csrc/ops_cluster.hip).  Test infrastructure only: the product path never imports it.

Sources restated (reference tree):
  inst/include/FactorNet/clustering/bipartition.hpp
    :33-50   centroid(): column sums over the sample list, then `/= samples.size()`
    :68-90   compute_centroid() (dclust leaves): the same sums, then `*= 1 / samples.size()`
    :93-126  rel_cosine(): per sample sqrt(x.c_other) |c_own| / (sqrt(x.c_own) |c_other|), summed, / (2 * rows)
    :161-169 scale(): d = row sums + 1e-15 (core/constants.hpp tiny_num<double>), rows divided by d
    :172-194 cor(): 1 - Pearson over all 2 x m entries of w against the previous w
    :197-233 nnls2 / nnls2InPlace: closed-form 2 x 2 solve, std::max(0.0, x) under nonneg
    :241-338 c_bipartition_sparse(): the ALS loop, orientation by d, the split
    :420-447 bipartition(): w (2 x rows) from SplitMix64(seed) uniform() draws, row 0 first
  inst/include/FactorNet/clustering/dclust.hpp:69-140  the LIFO driver, same seed for every split
"""
import numpy as np

from rcppml_amd.data import splitmix64_uniform

TINY = 1e-15


def _cmax0(x):
    """std::max(0.0, x): returns 0.0 unless 0.0 < x -- so NaN maps to 0, -0.0 to 0.0."""
    x = np.asarray(x, np.float64)
    return np.where(0.0 < x, x, 0.0)


def _csc(A):
    import scipy.sparse as sp
    A = sp.csc_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


def init_w(seed, m):
    return splitmix64_uniform(int(seed), 0, 2 * m).reshape(2, m)


def _cor(w, w_it):
    n = float(w.size)
    x, y = w_it.ravel(), w.ravel()
    sxy, sx, sy, sxx, syy = float(x @ y), float(x.sum()), float(y.sum()), float(x @ x), float(y @ y)
    num = n * sxy - sx * sy
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt((n * sxx - sx * sx) * (n * syy - sy * sy))
        return float(1.0 - num / den)


def _solve2(a, b0, b1, nonneg):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        denom = a[0, 0] * a[1, 1] - a[0, 1] * a[0, 1]
        x0 = (b0 * a[1, 1] - b1 * a[0, 1]) / denom
        x1 = (b1 * a[0, 0] - b0 * a[0, 1]) / denom
    if nonneg:
        x0, x1 = _cmax0(x0), _cmax0(x1)
    return x0, x1


def _scale(x):
    d = x.sum(axis=1) + TINY
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / d[:, None], d


def centroid(A, samples, inverse=False):
    """bipartition.hpp:33-50 (inverse=False) and :68-90 (inverse=True, dclust leaves)."""
    s = np.asarray(A[:, samples].sum(axis=1)).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        if inverse:
            return s * (1.0 / float(len(samples)))
        return s / float(len(samples))


def rel_cosine(A, s1, s2, c1, c2):
    n1, n2 = np.sqrt(c1 @ c1), np.sqrt(c2 @ c2)
    with np.errstate(invalid="ignore", divide="ignore"):
        x1 = A[:, s1].T
        a11, a12 = x1 @ c1, x1 @ c2
        x2 = A[:, s2].T
        a21, a22 = x2 @ c1, x2 @ c2
        d1 = float(np.sum(np.sqrt(a12) * n1 / (np.sqrt(a11) * n2)))
        d2 = float(np.sum(np.sqrt(a21) * n2 / (np.sqrt(a22) * n1)))
    return (d1 + d2) / (2 * A.shape[0])


def bipartition(A, samples=None, tol=1e-5, maxit=100, nonneg=True, seed=0, calc_dist=True):
    """Returns dict(v, dist, size1, size2, samples1, samples2, center1, center2, iter, h, d)."""
    A = _csc(A)
    m, n = A.shape
    samples = np.arange(n) if samples is None else np.asarray(samples, np.int64)
    if maxit < 1:
        raise ValueError("maxit must be at least 1")
    As = A[:, samples]                     # duplicates allowed: a repeated sample is a repeated column
    AsT = As.T.tocsr()
    w = init_w(seed, m)
    tol_, it = 1.0, 0
    h = np.zeros((2, len(samples)))
    d = np.ones(2)
    while it < maxit and tol_ > tol:
        w_it = w.copy()
        a = w @ w.T
        b = AsT @ w.T                      # (n_sub, 2)
        h0, h1 = _solve2(a, b[:, 0], b[:, 1], nonneg)
        h, d = _scale(np.vstack([h0, h1]))
        a = h @ h.T
        bw = As @ h.T                      # (m, 2): rows without a nonzero in the subset get b = 0
        w0, w1 = _solve2(a, bw[:, 0], bw[:, 1], nonneg)
        w, d = _scale(np.vstack([w0, w1]))
        tol_ = _cor(w, w_it)
        it += 1
    v = h[0] - h[1] if d[0] > d[1] else h[1] - h[0]
    pos = v > 0
    s1, s2 = samples[pos], samples[~pos]
    dist = -1.0
    c1 = c2 = np.zeros(m)
    if calc_dist:
        c1, c2 = centroid(A, s1), centroid(A, s2)
        dist = rel_cosine(A, s1, s2, c1, c2)
    return dict(v=v, dist=dist, size1=int(pos.sum()), size2=int((~pos).sum()), samples1=s1, samples2=s2, center1=c1,
                center2=c2, iter=it, h=h, d=d)


def dclust(A, min_samples, min_dist=0.0, tol=1e-5, maxit=100, nonneg=True, seed=0, splits=None):
    """dclust.hpp:69-140.  Returns the leaves in emission order: list of dict(samples, center, id, size, radius).
    `splits` (a list) receives every bipartition result together with its parent's sample set."""
    A = _csc(A)
    if min_samples < 1:
        raise ValueError("min_samples must be at least 1")
    calc_dist = min_dist > 0
    stack = [(np.arange(A.shape[1]), "")]
    out = []
    while stack:
        s, path = stack.pop()
        if len(s) < 2 * min_samples:
            out.append(dict(samples=s, center=centroid(A, s, inverse=True), id=path, size=len(s), radius=0.0))
            continue
        r = bipartition(A, s, tol=tol, maxit=maxit, nonneg=nonneg, seed=seed, calc_dist=calc_dist)
        if splits is not None:
            splits.append(dict(parent=s, **r))
        ok = r["size1"] >= min_samples and r["size2"] >= min_samples
        if ok and calc_dist and r["dist"] < min_dist:
            ok = False
        if ok:
            stack.append((r["samples1"], path + "0"))
            stack.append((r["samples2"], path + "1"))
        else:
            out.append(dict(samples=s, center=centroid(A, s, inverse=True), id=path, size=len(s),
                            radius=r["dist"] if calc_dist else 0.0))
    return out
