"""Plain float64 numpy restatement of the per-column coordinate-descent NNLS solve and of the explicit-mask half-update -- the
parity target of rcppml_hip_solve_cd and rcppml_hip_solve_masked.  Test infrastructure only: no torch, no GPU code, no oracle;
tests/test_cd_ref_cpu.py pins it to the oracle (fp64), the GPU tests compare every kernel with it.

Semantics restated (include/rcppml_gpu.h, "Per-column CD NNLS"; reference primitives/cpu/nnls_batch.hpp:70-132
cd_nnls_col_fixed with the prologues of fused_nnls.hpp:116-123 / nnls_batch.hpp:167-174, and nmf/masked_nnls.hpp:96-154):
  b = B(:,j); if (l1_pre > 0) b -= l1_pre; x = zero_init ? 0 : X(:,j); if (warm) b -= G x;
  per sweep, per coordinate i in order:  skip when G_ii <= 0;  diff = b_i / G_ii - l1 + l2 * x_i  (the reference ADDS l2 x_i);
    clip x_i + diff to 0 (nonneg) and then to ub; skip zero steps;  b -= G(:,i) a_i
  stop after the sweep in which  sum_i |a_i| / (|x_i| + 1e-15) * (1 / k) < tol  (tol > 0 only), at the latest after maxit sweeps;
  if (ub_post > 0) x = min(x, ub_post).
Everything runs in float64 whatever the dtype of the inputs: for fp32 kernels this is a high-precision reference of the same
operation on the same (fp32-rounded) inputs, not a second fp32 computation.
"""
import numpy as np


def cd_solve(G, b, x0, *, l1_pre=0.0, warm=False, zero_init=False, l1_cd=0.0, l2_cd=0.0, nonneg=True, maxit=100, tol=0.0,
             ub_cd=0.0, ub_post=0.0):
    """One column.  Returns (x, sweeps, stat): stat[s] = the stop statistic of sweep s (computed whether or not tol > 0; a value
    of 0 means that no coordinate moved in that sweep)."""
    G = np.asarray(G, np.float64)
    k = G.shape[0]
    b = np.array(b, np.float64)
    if l1_pre > 0:
        b -= l1_pre
    x = np.zeros(k) if zero_init else np.array(x0, np.float64)
    if warm:
        for c in range(k):
            b -= G[c] * x[c]
    inv_k = 1.0 / k
    stat = []
    sweeps = maxit
    for it in range(maxit):
        tol_sum = 0.0
        for i in range(k):
            g = G[i, i]
            if g <= 0:
                continue
            diff = b[i] / g
            if l1_cd != 0:
                diff -= l1_cd
            if l2_cd != 0:
                diff += l2_cd * x[i]
            nv = x[i] + diff
            if nonneg and nv < 0:
                a = -x[i]
                nx = 0.0
            elif ub_cd > 0 and nv > ub_cd:
                a = ub_cd - x[i]
                nx = ub_cd
            else:
                a = diff
                nx = nv
            if a == 0:
                continue
            x[i] = nx
            tol_sum += abs(a) / (abs(nx) + 1e-15)
            b -= G[i] * a
        stat.append(tol_sum * inv_k)
        if tol > 0 and tol_sum * inv_k < tol:
            sweeps = it + 1
            break
    if ub_post > 0:
        x = np.minimum(x, ub_post)
    return x, sweeps, np.asarray(stat)


def cd_solve_batch(G, B, X0, *, l1_pre=0.0, warm=False, zero_init=False, l1_cd=0.0, l2_cd=0.0, nonneg=True, maxit=100, tol=0.0,
                   ub_cd=0.0, ub_post=0.0):
    """cd_solve on every row of B / X0 (shape (n, k): row j = column j of the k x n matrices).  The columns are independent and
    every one goes through the same elementwise float64 operations in the same order as in cd_solve, so the results are bit for bit
    those of n calls (tests/test_cd_ref_cpu.py checks that); the loop over columns is only vectorised.  G is one k x k Gram for
    all columns or, shape (n, k, k), one per column (the explicit-mask half-update).  Returns (X, sweeps (n,), stat (n, maxit), NaN
    after a column's last sweep)."""
    G = np.asarray(G, np.float64)
    own = G.ndim == 3
    k = G.shape[-1]
    B = np.array(B, np.float64)
    n = B.shape[0]
    if l1_pre > 0:
        B -= l1_pre
    X = np.zeros((n, k)) if zero_init else np.array(X0, np.float64)
    if warm:
        for c in range(k):
            B -= (G[:, c] if own else G[c][None, :]) * X[:, c][:, None]
    inv_k = 1.0 / k
    stat = np.full((n, max(maxit, 0)), np.nan)
    sweeps = np.full(n, maxit, np.int64)
    act = np.ones(n, bool)
    for it in range(maxit):
        idx = np.nonzero(act)[0]
        if idx.size == 0:
            break
        Bs, Xs = B[idx], X[idx]
        Gs = (G if idx.size == n else G[idx]) if own else None
        tol_sum = np.zeros(idx.size)
        for i in range(k):
            g = Gs[:, i, i] if own else G[i, i]
            ok = g > 0
            if not np.any(ok):
                continue
            xi = Xs[:, i]
            diff = Bs[:, i] / np.where(ok, g, 1.0)
            if l1_cd != 0:
                diff = diff - l1_cd
            if l2_cd != 0:
                diff = diff + l2_cd * xi
            nv = xi + diff
            a, nx = diff, nv
            if ub_cd > 0:
                up = nv > ub_cd
                a = np.where(up, ub_cd - xi, a)
                nx = np.where(up, ub_cd, nx)
            if nonneg:
                neg = nv < 0
                a = np.where(neg, -xi, a)
                nx = np.where(neg, 0.0, nx)
            mv = (a != 0) & ok
            a = np.where(mv, a, 0.0)
            Xs[:, i] = np.where(mv, nx, xi)
            tol_sum += np.where(mv, np.abs(a) / (np.abs(nx) + 1e-15), 0.0)
            Bs -= a[:, None] * (Gs[:, i] if own else G[i][None, :])
        B[idx], X[idx] = Bs, Xs
        st = tol_sum * inv_k
        stat[idx, it] = st
        if tol > 0:
            done = st < tol
            sweeps[idx[done]] = it + 1
            act[idx[done]] = False
    if ub_post > 0:
        X = np.minimum(X, ub_post)
    return X, sweeps, stat


def decisive(stat, tol, delta):
    """Columns whose stop statistic lies outside tol * (1 +- delta) at every sweep they ran: their sweep count cannot depend on
    rounding of relative size delta in the statistic."""
    s = np.where(np.isnan(stat), np.inf, stat)
    return ~np.any((s > tol * (1 - delta)) & (s < tol * (1 + delta)), axis=1)


def masked_half_update(A, M, F, G, X0, *, l1=0.0, l2=0.0, nonneg=True, maxit=100, tol=1e-8, solver_mode=0, warm=False):
    """Explicit-mask half-update (nmf/masked_nnls.hpp:96-154).  A, M: CSC with attributes p, i, x (M: every stored entry is a
    masked row of that column); F: (rows, k); G: k x k Gram of F; X0: (cols, k).  Per column j: b = sum over the stored entries
    that are not masked of a f_row; G_loc = G - sum over ALL masked rows of f f^T + l2 I; b -= l1; x = X0(j) if warm else 0 (no
    residual correction); then cd_solve (all columns at once: cd_solve_batch with one Gram per column), or clip(G_loc^-1 b)
    (numpy.linalg.solve) when solver_mode == 1."""
    F = np.asarray(F, np.float64)
    G = np.asarray(G, np.float64)
    k = F.shape[1]
    n = len(A.p) - 1
    Bl = np.zeros((n, k))
    Gl = np.repeat(G[None], n, axis=0)
    for j in range(n):
        mrows = np.asarray(M.i[M.p[j]:M.p[j + 1]], np.int64)
        masked = set(mrows.tolist())
        for t in range(A.p[j], A.p[j + 1]):
            if int(A.i[t]) in masked:
                continue
            Bl[j] += float(A.x[t]) * F[A.i[t]]
        for r in mrows:
            Gl[j] -= np.outer(F[r], F[r])
    Bl -= l1
    Gl[:, np.arange(k), np.arange(k)] += l2
    if solver_mode == 1:
        X = np.stack([np.linalg.solve(Gl[j], Bl[j]) for j in range(n)])
        return np.maximum(X, 0.0) if nonneg else X
    X0 = np.asarray(X0, np.float64) if warm else np.zeros((n, k))
    return cd_solve_batch(Gl, Bl, X0, nonneg=nonneg, maxit=maxit, tol=tol)[0]
