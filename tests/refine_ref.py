"""Plain numpy restatement of the reference's compute_target() (R/compute_target.R:65-121) and refine() without a batch
(R/refine.R:109-187), written from the R text; the tests compare the HIP path (rcppml_amd/csrc/ops_refine.hip) with it.

compute_target: class sums over the columns in column order, divided by the counts (an empty class keeps a zero centroid);
             grand_mean = the mean of the non-empty classes' centroids; with whiten and C > 1: X = (centroids - grand_mean) *
             sqrt(max(count, 1)), S = X X^T / sum(count), the OAS rho with (1 - 2/k) as written, rho = 1 when |rho_den| < 1e-12,
             S_shrunk = (1 - rho) S + rho tr(S)/k I, eigenvalues floored at 1e-10, W_zca = V diag(1/sqrt(vals)) V^T applied to the
             centroids and grand_mean; target[, j] = centroid[label_j] - grand_mean, zero for NA.
stage 1:     T scaled by ||H||_F / ||T||_F when ||T||_F > 1e-10, H + lambda T, clipped at 0 when nonneg.
cycle:       W = solve(G + 1e-8 I, B) with dH = diag(d) H_corr, G = dH dH^T, B = A dH^T, clip; H = solve(W^T W + 1e-8 I, W^T A), clip;
             d = row norms of H floored at 1e-10, H / d, W * d; stage 1 on the new H.

Labels are integer codes 0 .. C - 1 with a negative code for NA (rcppml_amd.refine.as_factor makes them).  Matrices: H k x n,
W m x k, A m x n dense.

variant=True is the same arithmetic with the columns visited in reverse order and every accumulation (sums, products, norms) in
np.longdouble, rounded to double where R holds a double: the tests take the difference between the two as the scale of what a
change of summation order does to each output.
"""
import numpy as np

LD = np.longdouble


def _mm(X, Y, variant):
    """X @ Y; the variant contracts in reverse order in long double."""
    if not variant:
        return X @ Y
    return (np.ascontiguousarray(X[:, ::-1]).astype(LD) @ np.ascontiguousarray(Y[::-1, :]).astype(LD)).astype(np.float64)


def _sumsq(X, variant):
    if not variant:
        return float(np.sum(X ** 2))
    return float(np.sum((X.astype(LD) ** 2).ravel()[::-1]))


def kc_stage(centroids, counts, whiten=True, variant=False, detail=None):
    """shift (k x C) from the class centroids and counts (R/compute_target.R:81-115)."""
    k, C = centroids.shape
    counts = np.asarray(counts)
    ne = counts > 0
    if variant:
        gm = (np.sum(centroids[:, ne].astype(LD)[:, ::-1], axis=1) / LD(int(ne.sum()))).astype(np.float64) if ne.any() \
            else np.full(k, np.nan)
    else:
        gm = centroids[:, ne].mean(axis=1) if ne.any() else np.full(k, np.nan)
    if whiten and C > 1:
        wts = np.sqrt(np.maximum(counts, 1).astype(np.float64))
        X = (centroids - gm[:, None]) * wts[None, :]
        n_eff = float(counts.sum())
        S = _mm(X, X.T, variant) / n_eff
        trS = float(np.trace(S))
        trS2 = float(np.sum(S * S))
        rho_num = (1 - 2 / k) * trS2 + trS ** 2
        rho_den = (n_eff + 1 - 2 / k) * (trS2 - trS ** 2 / k)
        rho = 1.0 if abs(rho_den) < 1e-12 else min(1.0, max(0.0, rho_num / rho_den))
        S_shrunk = (1 - rho) * S + rho * (trS / k) * np.eye(k)
        vals, V = np.linalg.eigh(S_shrunk)
        floored = vals < 1e-10
        vals = np.maximum(vals, 1e-10)
        W_zca = _mm(V * (1 / np.sqrt(vals))[None, :], V.T, variant)
        if detail is not None:
            detail.update(S_shrunk=S_shrunk, W_zca=W_zca, rho=rho, vals=vals, floored=floored)
        centroids = _mm(W_zca, centroids, variant)
        gm = _mm(W_zca, gm[:, None], variant)[:, 0]
    return centroids - gm[:, None]


def class_centroids(H, codes, C, variant=False):
    k, n = H.shape
    acc = LD if variant else np.float64
    cen = np.zeros((k, C), acc)
    counts = np.zeros(C, np.int64)
    for j in (range(n - 1, -1, -1) if variant else range(n)):
        ci = codes[j]
        if ci >= 0:
            cen[:, ci] += H[:, j]
            counts[ci] += 1
    for ci in range(C):
        if counts[ci] > 0:
            cen[:, ci] /= counts[ci]
    return cen.astype(np.float64), counts


def compute_target(H, codes, C, whiten=True, variant=False, detail=None):
    H = np.asarray(H, np.float64)
    codes = np.asarray(codes)
    k, n = H.shape
    cen, counts = class_centroids(H, codes, C, variant)
    T = np.zeros((k, n))
    if C == 0:
        return T
    shift = kc_stage(cen, counts, whiten, variant, detail)
    lab = codes >= 0
    T[:, lab] = shift[:, codes[lab]]
    return T


def stage1(H, codes, C, lam, nonneg=True, whiten=True, variant=False):
    T = compute_target(H, codes, C, whiten, variant)
    fro_H = np.sqrt(_sumsq(H, variant))
    fro_T = np.sqrt(_sumsq(T, variant))
    if fro_T > 1e-10:
        T = T * (fro_H / fro_T)
    Hc = H + lam * T
    if nonneg:
        Hc[Hc < 0] = 0
    return Hc


def w_refit(A, d, H_corr, nonneg=True, variant=False):
    """W (m x k) of R/refine.R:137-145."""
    k = H_corr.shape[0]
    dH = d[:, None] * H_corr
    G = _mm(dH, dH.T, variant)
    B = _mm(A, dH.T, variant)
    W = np.linalg.solve(G + 1e-8 * np.eye(k), B.T).T
    if nonneg:
        W[W < 0] = 0
    return W


def refine(W, d, H, A, codes, C, lam=0.8, cycles=0, nonneg=True, whiten=True, variant=False):
    """(W, d, H, H_corr) after `cycles` cycles; W and d are returned untouched when cycles = 0."""
    W = None if W is None else np.array(W, np.float64)
    d = None if d is None else np.array(d, np.float64)
    H = np.array(H, np.float64)
    k = H.shape[0]
    Hc = stage1(H, codes, C, lam, nonneg, whiten, variant)
    for _ in range(int(cycles)):
        W = w_refit(A, d, Hc, nonneg, variant)
        WtW = _mm(W.T, W, variant)
        WtA = _mm(A.T, W, variant)
        H = np.linalg.solve(WtW + 1e-8 * np.eye(k), WtA.T)
        if nonneg:
            H[H < 0] = 0
        d = np.sqrt(np.array([_sumsq(H[f], variant) for f in range(k)]))
        d[d < 1e-10] = 1e-10
        H = H / d[:, None]
        W = W * d[None, :]
        Hc = stage1(H, codes, C, lam, nonneg, whiten, variant)
    return W, d, H, Hc


def rel_diff(a, b):
    """max |a - b| / max |b| (0 when both are all zero): the measure of the parity tests."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.max(np.abs(b))) if b.size else 0.0, float(np.max(np.abs(a))) if a.size else 0.0)
    return 0.0 if scale == 0 else float(np.max(np.abs(a - b))) / scale


def within_class_cosine(H, codes):
    """Mean over the classes with >= 2 members of the mean pairwise cosine similarity of their columns."""
    H = np.asarray(H, np.float64)
    codes = np.asarray(codes)
    out = []
    for c in np.unique(codes[codes >= 0]):
        X = H[:, codes == c]
        if X.shape[1] < 2:
            continue
        nrm = np.sqrt((X ** 2).sum(axis=0))
        Xn = X / np.where(nrm > 0, nrm, 1.0)
        S = Xn.T @ Xn
        q = X.shape[1]
        out.append((S.sum() - np.trace(S)) / (q * (q - 1)))
    return float(np.mean(out))
