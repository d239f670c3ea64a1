"""numpy specification of the similarity entries (csrc/ops_similarity.hip) and of cosine() / bipartiteMatch() / align()
(rcppml_amd/similarity.py).  Plain fp64 numpy, no device.

What the device computes (include/rcppml_gpu.h has the contracts):
  sparse cosine   C[i, j] = dot(x_i, y_j) / (|x_i| * |y_j|), 0 where the norm product is 0.  dot: the products of the rows both
                  columns store, added in ascending row order from 0; |x|: the squares added in ascending row order, square root.
                  Every product and sum is rounded on its own (no FMA).  cosine_sequential() restates exactly that order.
  dense cosine    the same value with the sum over the m rows taken in fixed chunks (dot) and in a lane + butterfly order (means,
                  norms); method 1 (Pearson) centres the columns by their means first, never sum(xy) - m mean(x) mean(y).
  matching        minimum-cost assignment, negatives counted as 0, -1 for a row left unmatched (more rows than columns).

Zero-norm rule: a column of zero norm (zero centred norm for the correlation) has similarity 0 to every column, itself included.

The two deviations from R:
  1. cosine(vector x, matrix y): R/cosine.R:47 multiplies x by |x|^2 instead of dividing by |x|.  cosine_ref returns the cosine.
  2. align(): assignment[i] is the ref factor matched to object factor i; R/nmf_methods.R:270 indexes the object by that vector
     (the permutation, where its inverse is needed).  align_order() is argsort(assignment); align_order_literal_R() is R's reading,
     kept so that a test can show the difference on a 3-cycle.

Error bounds (u = 2^-53).
  Cosine.  A dot product of n terms summed in any order, fused or not, is off by at most gamma_n sum|x y| <= gamma_n |x| |y|
  (Higham, Accuracy and Stability, 3.1), gamma_n ~ n u, and n <= min(nnz_i, nnz_j).  A sum of squares of n terms has relative
  error gamma_n, its square root (n / 2 + 1) u; the norm product and the division add u each.  Against the exact value therefore
      |C_dev - C| <= (nnz_i + nnz_j + 8) u,
  with room to spare (min(nnz) + nnz_i / 2 + nnz_j / 2 + 4 is what the argument gives).  An fp64 numpy reference carries the same
  error, so a comparison with it uses twice the bound.  The dense entry: nnz replaced by m.
  Correlation.  Centring x - mean costs |x| u per entry relative to the centred norm |x - mean|, a factor rms / sd; with kappa the
  largest rms / sd over the columns the same form holds times kappa^2: (2 m + 8) kappa^2 u, doubled against fp64 numpy.
"""
import itertools

import numpy as np

U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------------------- bounds
def cosine_bound(nnz_x, nnz_y):
    """(nx, ny) bound of |C_dev - C_exact| from the stored entries per column."""
    return (np.asarray(nnz_x, dtype=np.float64)[:, None] + np.asarray(nnz_y, dtype=np.float64)[None, :] + 8.0) * U


def dense_bound(m, kappa=1.0):
    return (2.0 * m + 8.0) * float(kappa) ** 2 * U


def kappa(*mats):
    """Largest rms / sd over the columns of the matrices (columns of zero sd left out: their similarity is 0 by rule)."""
    k = 1.0
    for a in mats:
        a = np.asarray(a, dtype=np.float64)
        rms = np.sqrt(np.mean(a * a, axis=0))
        sd = np.sqrt(np.mean((a - a.mean(axis=0)) ** 2, axis=0))
        ok = sd > 0
        if ok.any():
            k = max(k, float(np.max(rms[ok] / sd[ok])))
    return k


# ------------------------------------------------------------------------------------------------------------- cosines
def _scipy(a):
    import scipy.sparse as sp
    if hasattr(a, "to_scipy"):
        return a.to_scipy()
    return a.tocsc() if hasattr(a, "tocsc") else sp.csc_matrix(np.asarray(a, dtype=np.float64))


def normalise(dot, nx, ny):
    den = nx[:, None] * ny[None, :]
    out = np.zeros_like(dot)
    np.divide(dot, den, out=out, where=den > 0)
    return out


def cosine_sparse_ref(x, y=None):
    """fp64 restatement of the sparse entry (numpy / scipy summation order): (nx, ny)."""
    X = _scipy(x)
    Y = X if y is None else _scipy(y)
    if X.shape[0] * (X.shape[1] + Y.shape[1]) <= 5e7:          # small: the dense product is the faster restatement
        dot = X.toarray().T @ Y.toarray()
    else:
        dot = np.asarray((X.T @ Y).todense(), dtype=np.float64)
    nx =np.sqrt(np.asarray(X.multiply(X).sum(axis=0)).ravel())
    ny = np.sqrt(np.asarray(Y.multiply(Y).sum(axis=0)).ravel())
    return normalise(dot, nx, ny)


def cosine_sequential(x, y=None, dtype=np.float64):
    """The device's own order, entry by entry (slow: small inputs only).  dtype=np.longdouble gives the near-exact value."""
    X = _scipy(x)
    Y = X if y is None else _scipy(y)
    X.sort_indices()
    Y.sort_indices()
    zero = dtype(0)

    def norms(A):
        out = np.zeros(A.shape[1], dtype)
        for j in range(A.shape[1]):
            s = zero
            for v in A.data[A.indptr[j]:A.indptr[j + 1]]:
                s = s + dtype(v) * dtype(v)
            out[j] = np.sqrt(s)
        return out

    nx, ny = norms(X), norms(Y)
    C = np.zeros((X.shape[1], Y.shape[1]), dtype)
    for j in range(Y.shape[1]):
        rows_y = Y.indices[Y.indptr[j]:Y.indptr[j + 1]]
        vals_y = Y.data[Y.indptr[j]:Y.indptr[j + 1]]
        for i in range(X.shape[1]):
            rows_x = X.indices[X.indptr[i]:X.indptr[i + 1]]
            vals_x = X.data[X.indptr[i]:X.indptr[i + 1]]
            common, ix, iy = np.intersect1d(rows_x, rows_y, assume_unique=True, return_indices=True)
            s = zero
            for a, b in zip(vals_x[ix], vals_y[iy]):
                s = s + dtype(b) * dtype(a)
            den = nx[i] * ny[j]
            C[i, j] = s / den if den > 0 else zero
    return C


def cosine_dense_ref(W, R, method="cosine"):
    """fp64 restatement of the dense entry.  W: (reps, m, kx) or (m, kx); R: (m, ky).  Returns (reps, kx, ky) or (kx, ky)."""
    W = np.asarray(W, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    if W.ndim == 2:
        return cosine_dense_ref(W[None], R, method)[0]
    if method in ("cor", 1):
        W = W - W.mean(axis=1, keepdims=True)
        R = R - R.mean(axis=0, keepdims=True)
    nr = np.sqrt(np.sum(R * R, axis=0))
    return np.stack([normalise(w.T @ R, np.sqrt(np.sum(w * w, axis=0)), nr) for w in W])


def cosine_ref(x, y=None):
    """The R surface: shapes and the vector rules of cosine()."""
    def is_vec(a):
        return not hasattr(a, "tocsc") and not hasattr(a, "to_scipy") and np.ndim(a) == 1

    if y is None and is_vec(x):
        raise ValueError("x is a vector and y is NULL")
    xv, yv = is_vec(x), (y is not None and is_vec(y))
    X = np.asarray(x, dtype=np.float64).reshape(-1, 1) if xv else x
    Y = np.asarray(y, dtype=np.float64).reshape(-1, 1) if yv else y
    out = cosine_sparse_ref(X, Y)
    if xv and yv:
        return float(out[0, 0])
    return out.reshape(-1) if (xv or yv) else out


# ------------------------------------------------------------------------------------------------------------- matching
def clip_cost(cost):
    c = np.array(cost, dtype=np.float64)
    c[c < 0] = 0.0
    return c


def match_bruteforce(cost):
    """(assignment, cost) by enumeration: every injective map of the shorter side into the longer one.  -1: unmatched row."""
    c = clip_cost(cost)
    nr, nc = c.shape
    best, best_a = np.inf, None
    if nr <= nc:
        for perm in itertools.permutations(range(nc), nr):
            s = sum(c[i, perm[i]] for i in range(nr))
            if s < best:
                best, best_a = s, np.array(perm)
    else:
        for perm in itertools.permutations(range(nr), nc):          # perm[j]: the row column j takes
            s = sum(c[perm[j], j] for j in range(nc))
            if s < best:
                best = s
                best_a = np.full(nr, -1)
                best_a[list(perm)] = np.arange(nc)
    return best_a, float(best)


def match_ref(cost):
    """Shortest augmenting paths with dual potentials (Jonker-Volgenant / Hungarian), the entry's algorithm restated."""
    c = clip_cost(cost)
    nr, nc = c.shape
    a = c if nr <= nc else c.T
    n, m = a.shape
    u, v = np.zeros(n + 1), np.zeros(m + 1)
    p, way = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0, delta, j1 = p[j0], np.inf, 0
            for j in range(1, m + 1):
                if used[j]:
                    continue
                cur = a[i0 - 1, j - 1] - u[i0] - v[j]
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                if minv[j] < delta:
                    delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    row_of = p[1:] - 1                      # the row of `a` matched to its column j, -1 for none
    if nr <= nc:
        assignment = np.full(nr, -1)
        for j, r in enumerate(row_of):
            if r >= 0:
                assignment[r] = j
    else:
        assignment = row_of.copy()
    total = float(sum(c[i, assignment[i]] for i in range(nr) if assignment[i] >= 0))
    return assignment, total


# ------------------------------------------------------------------------------------------------------------- align
def similarity_cost(sim):
    cost = 1.0 - np.asarray(sim, dtype=np.float64) + 1e-10
    cost[cost < 0] = 0.0
    return cost


def align_order(assignment):
    """aligned factor j = the object factor matched to ref factor j."""
    return np.argsort(np.asarray(assignment), kind="stable")


def align_order_literal_R(assignment):
    """R/nmf_methods.R:270: object[assignment + 1L]."""
    return np.asarray(assignment).copy()


def align_ref(w_obj, w_ref, method="cosine", order_rule=align_order):
    """(order, assignment) for one pair of m x k loadings."""
    sim = cosine_dense_ref(w_obj, w_ref, method)
    assignment, _ = match_ref(similarity_cost(sim))
    return order_rule(assignment), assignment
