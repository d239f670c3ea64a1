"""numpy restatement of the reference's constrained block SVD, Krylov-Seeded Projected Refinement (krylov_constrained_svd_impl,
inst/include/FactorNet/svd/krylov.hpp:262-796), for the scope of the GPU entries rcppml_gpu_svd_krylov_ex / _dense_ex: L1, L2,
nonneg and upper bound on either side, centering, FACTOR convergence, a given seed V0.  Test infrastructure only (like svd_ref.py):
the parity target of tests/test_gpu_svd_krylov.py, checked on its own in tests/test_svd_krylov_cpu.py.

The k x k system is solved in float64 in every dtype; everything else runs in `dtype` (np.float32, np.float64 or np.longdouble)."""
import functools

import numpy as np


def pass_limit(k, max_iter=0):
    """krylov.hpp:428-431."""
    return int(max_iter) if max_iter > 0 else max(10, 2 * int(np.ceil(np.log2(k))) + 3)


def project_and_normalize(X, L1, nonneg, ub, nsq, eps100):
    """krylov.hpp:162-210 with L2 = 0 (:515-524: L2 is in the Gram, not applied again).  X: rows x k, changed in place; returns d."""
    dt = X.dtype.type
    d = np.zeros(X.shape[1], X.dtype)
    for c in range(X.shape[1]):
        if not nsq[c] > 0:                                                  # :175-179
            X[:, c] = 0
            continue
        x = X[:, c]
        if L1 > 0:                                                          # :188-196
            thr = dt(L1) / (dt(2) * nsq[c])
            x = np.where(x > thr, x - thr, np.where(x < -thr, x + thr, dt(0))).astype(X.dtype)
        if nonneg:                                                          # :199
            x = np.maximum(x, dt(0))
        if ub > 0:                                                          # :202-203
            x = np.minimum(x, dt(ub))
        nrm = np.sqrt(np.sum(x * x, dtype=X.dtype))                          # :206-208
        d[c] = nrm if nrm > eps100 else dt(0)
        X[:, c] = x / d[c] if d[c] > 0 else x
    return d


def half_update(A, F, L1, L2, nonneg, ub, eps100, center_term=None, pass_no=0, side="W"):
    """One side of a pass (krylov.hpp:472-524 / :535-580): X = proj(A F (F'F + (1e-12 + L2) I)^-1).  center_term(F): the rows x k
    matrix subtracted from A F.  Raises ValueError on a Gram matrix that is not positive definite."""
    dt = A.dtype.type
    G = (F.T @ F).astype(A.dtype)
    nsq = np.diag(G).copy()
    G[np.diag_indices_from(G)] += dt(1e-12) + dt(L2)
    B = (A @ F).astype(A.dtype)
    if center_term is not None:
        B = B - center_term(F)
    try:
        np.linalg.cholesky(G.astype(np.float64))
    except np.linalg.LinAlgError:
        raise ValueError("non-positive Cholesky pivot in pass %d, %s-update" % (pass_no + 1, side))
    X = np.linalg.solve(G.astype(np.float64), B.astype(np.float64).T).T.astype(A.dtype)
    d = project_and_normalize(X, L1, nonneg, ub, nsq, eps100)
    return X, d


def extract(W, d, V):
    """krylov.hpp:216-247 in float64: QR of W diag(d) and of V, SVD of R_w R_v'.  Column signs are the factorisation's."""
    Qw, Rw = np.linalg.qr(np.asarray(W, np.float64) * np.asarray(d, np.float64))
    Qv, Rv = np.linalg.qr(np.asarray(V, np.float64))
    Us, s, Vst = np.linalg.svd(Rw @ Rv.T)
    return Qw @ Us, s, Qv @ Vst.T


def phase3(W, d, V, hard):
    """krylov.hpp:742-781: with a hard constraint the factors by d descending (ties by index), else the QR extraction."""
    if hard:
        order = sorted(range(len(d)), key=lambda c: (-float(d[c]), c))
        return W[:, order].astype(np.float64), d[order].astype(np.float64), V[:, order].astype(np.float64)
    return extract(W, d, V)


def kspr(A, V0, max_passes=0, tol=0.0, L1=(0.0, 0.0), L2=(0.0, 0.0), nonneg=(False, False), ub=(0.0, 0.0), center=False,
         dtype=np.float64):
    """Phase 2 and 3 from the seed V0 (n x k; only V of a seed is read: the first W-update overwrites W and d).
    Returns dict(W, d, V: the Phase-2 factors; dw: the dW of each pass from the second on; passes; u, s, v: the Phase-3 result)."""
    A = np.asarray(A, dtype)
    V = np.asarray(V0, dtype).copy()
    k = V.shape[1]
    dt = A.dtype.type
    eps = dt(np.finfo(dtype).eps)
    eps100 = eps * dt(100)
    mu = np.asarray(np.asarray(A, np.float64).mean(axis=1), dtype) if center else None
    cw = (lambda F: np.outer(mu, F.sum(axis=0, dtype=A.dtype))) if center else None            # mu (1'V)
    cv = (lambda F: np.outer(np.ones(A.shape[1], A.dtype), mu @ F)) if center else None         # 1 (mu'W)
    limit = pass_limit(k, max_passes)
    At = np.ascontiguousarray(A.T)
    dws, prev, passes = [], None, 0
    for p in range(limit):
        W, d = half_update(A, V, L1[0], L2[0], nonneg[0], ub[0], eps100, cw, p, "W")
        V, d = half_update(At, W, L1[1], L2[1], nonneg[1], ub[1], eps100, cv, p, "V")
        passes = p + 1
        if p > 0:                                                                             # :588-601, FACTOR
            dW = np.sqrt(np.sum((W - prev) ** 2, dtype=A.dtype)) / (np.sqrt(np.sum(prev * prev, dtype=A.dtype)) + eps)
            dws.append(dW)
            if dW < dt(tol):
                break
        prev = W
    hard = bool(nonneg[0] or nonneg[1] or L1[0] > 0 or L1[1] > 0 or ub[0] > 0 or ub[1] > 0)
    u, s, v = phase3(W, d, V, hard)
    return dict(W=W, d=d, V=V, dw=np.asarray(dws, np.float64), passes=passes, u=u, s=s, v=v)


# ------------------------------------------------------------------------------------------------------------ test inputs
SHAPES = [(70, 45, 1), (70, 45, 8), (130, 67, 16), (130, 67, 17), (200, 150, 64), (200, 150, 65), (200, 150, 128)]
CONSTRAINTS = {
    "nonneg": dict(nonneg=(True, True)),
    "l1": dict(L1=(0.02, 0.02)),
    "nnu_l2_ubu": dict(nonneg=(True, False), L2=(0.1, 0.1), ub=(0.5, 0.0)),
    "nonneg_center": dict(nonneg=(True, True), center=True),
    "l2": dict(L2=(0.1, 0.1)),
}
PASSES = 5


@functools.lru_cache(maxsize=None)
def case_input(m, n):
    """Gamma-valued at density 0.25, one empty row and one empty column.  Returns (A, Vt of numpy's SVD)."""
    rng = np.random.default_rng(7000 + m)
    A = rng.gamma(2.0, 1.0, (m, n)) * (rng.random((m, n)) < 0.25)
    A[3, :] = 0
    A[:, 5] = 0
    return A, np.linalg.svd(A, full_matrices=False)[2]


def seed_of(m, n, k):
    """numpy's top-k right singular vectors with their signs fixed (LAPACK's are arbitrary): every column gets a non-negative sum,
    and for k > 1 the leading one, all of one sign on a non-negative matrix, enters negated, so that a nonneg projection kills it
    and the dead-column rule is exercised (a single factor is left alive)."""
    V = case_input(m, n)[1][:k].T
    V = V * np.where(V.sum(axis=0) < 0, -1.0, 1.0)
    if k > 1:
        V[:, 0] = -V[:, 0]
    return np.ascontiguousarray(V)


def convergence_input():
    """70 x 45 with a spectral gap after 8 values (50 .. 30, then 6 .. 0.5), a tenth of the entries zeroed, and a perturbed seed:
    under L2 only the passes contract like subspace iteration, so dW drops by more than ten from the second to the third pass.
    Returns (A, V0, k, tol, constraints)."""
    rng = np.random.default_rng(11)
    m, n, k = 70, 45, 8
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (U * np.concatenate([np.linspace(50, 30, k), np.linspace(6, 0.5, n - k)])) @ V.T
    A *= rng.random((m, n)) < 0.9
    Vt = np.linalg.svd(A, full_matrices=False)[2]
    V0, _ = np.linalg.qr(Vt[:k].T + 0.2 * rng.standard_normal((n, k)))
    return A, V0, k, 0.04, dict(L2=(0.01, 0.01))


def deviation(got, ref, align=False):
    """The largest of the four deviations between two results (dicts with u, s, v, dw): u, s and v relative to their largest reference
    magnitude; dw, itself a change relative to |W|, on its own scale (relative to max(1, largest reference dW): from an exact
    singular subspace under L2 only dW is rounding noise, and a relative deviation of noise says nothing).
    align: compare up to the sign of a column pair (the L2-only extraction)."""
    u, v = np.asarray(got["u"], np.float64), np.asarray(got["v"], np.float64)
    if align:
        sg = np.sign(np.sum(u * ref["u"], axis=0))
        sg[sg == 0] = 1
        u, v = u * sg, v * sg
    out = 0.0
    for a, b, floor in ((u, ref["u"], 0.0), (got["s"], ref["s"], 0.0), (v, ref["v"], 0.0), (got["dw"], ref["dw"], 1.0)):
        b = np.asarray(b, np.float64)
        if b.size:
            out = max(out, float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), floor, 1e-300)))
    return out


# The restatement's own deviations on each case at PASSES passes and tol = 0: (float32 run against the float64 run, float64 run
# against the np.longdouble run), by deviation().  The device is held to four times these (tests/test_gpu_svd_krylov.py).
# Regenerate with `python tests/svd_krylov_ref.py`.
MEASURED = {
    (70, 45, 1, 'nonneg'): (1.50e-07, 2.67e-16),
    (70, 45, 1, 'l1'): (1.21e-07, 2.05e-16),
    (70, 45, 1, 'nnu_l2_ubu'): (1.18e-07, 2.23e-16),
    (70, 45, 1, 'nonneg_center'): (3.11e-07, 5.92e-16),
    (70, 45, 1, 'l2'): (1.27e-07, 4.10e-16),
    (70, 45, 8, 'nonneg'): (3.20e-07, 8.37e-16),
    (70, 45, 8, 'l1'): (2.61e-07, 4.15e-16),
    (70, 45, 8, 'nnu_l2_ubu'): (1.83e-05, 3.08e-14),
    (70, 45, 8, 'nonneg_center'): (5.07e-07, 1.51e-15),
    (70, 45, 8, 'l2'): (1.02e-06, 1.34e-14),
    (130, 67, 16, 'nonneg'): (4.84e-07, 1.14e-15),
    (130, 67, 16, 'l1'): (3.08e-07, 7.57e-16),
    (130, 67, 16, 'nnu_l2_ubu'): (2.52e-04, 5.33e-13),
    (130, 67, 16, 'nonneg_center'): (2.09e-06, 1.66e-15),
    (130, 67, 16, 'l2'): (2.81e-06, 1.97e-13),
    (130, 67, 17, 'nonneg'): (5.19e-07, 1.01e-15),
    (130, 67, 17, 'l1'): (2.85e-07, 7.91e-16),
    (130, 67, 17, 'nnu_l2_ubu'): (7.64e-05, 1.11e-13),
    (130, 67, 17, 'nonneg_center'): (1.07e-06, 1.27e-15),
    (130, 67, 17, 'l2'): (1.78e-06, 1.46e-13),
    (200, 150, 64, 'nonneg'): (1.24e-06, 4.10e-15),
    (200, 150, 64, 'l1'): (3.57e-07, 8.03e-16),
    (200, 150, 64, 'nnu_l2_ubu'): (2.32e-04, 5.58e-13),
    (200, 150, 64, 'nonneg_center'): (7.85e-06, 8.71e-15),
    (200, 150, 64, 'l2'): (4.93e-06, 1.91e-13),
    (200, 150, 65, 'nonneg'): (1.42e-06, 4.97e-15),
    (200, 150, 65, 'l1'): (4.23e-07, 8.28e-16),
    (200, 150, 65, 'nnu_l2_ubu'): (3.39e-04, 5.89e-13),
    (200, 150, 65, 'nonneg_center'): (7.86e-06, 1.04e-14),
    (200, 150, 65, 'l2'): (3.52e-06, 1.81e-13),
    (200, 150, 128, 'nonneg'): (4.98e-05, 2.45e-13),
    (200, 150, 128, 'l1'): (7.90e-07, 2.08e-15),
    (200, 150, 128, 'nnu_l2_ubu'): (1.99e-04, 4.02e-13),
    (200, 150, 128, 'nonneg_center'): (1.26e-04, 3.34e-13),
    (200, 150, 128, 'l2'): (5.38e-06, 1.15e-13),
}


def measure():
    out = {}
    for m, n, k in SHAPES:
        A, V0 = case_input(m, n)[0], seed_of(m, n, k)
        for name, kw in CONSTRAINTS.items():
            r = {dt: kspr(A, V0, PASSES, 0.0, dtype=dt, **kw) for dt in (np.float32, np.float64, np.longdouble)}
            out[(m, n, k, name)] = (deviation(r[np.float32], r[np.float64], name == "l2"),
                                    deviation(r[np.float64], r[np.longdouble], name == "l2"))
    return out


if __name__ == "__main__":
    for key, (a, b) in measure().items():
        print("    %r: (%.2e, %.2e)," % (key, a, b))
