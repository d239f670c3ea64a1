"""Plain float64 numpy restatement of the sparse IRLS half-update -- the parity target of rcppml_hip_solve_irls.  Test
infrastructure only: no torch, no GPU code, no oracle; tests/test_irls_ref_cpu.py pins it to the oracle (fp64), the GPU tests
compare every kernel with it.

Semantics restated (reference primitives/cpu/nnls_batch_irls.hpp:202-329,465-520 with the weights of math/loss.hpp, as
rcppml_amd/csrc/kernels_irls.hip.h cites them).  Per column j, from x = 0, up to irls_max_iter passes:
  per stored entry (row, a):  mu = f_row . x;  w = weight(loss, a - mu, mu)
    loss 5 (NB):      r / (mu' (r + mu')) capped at 1e6, mu' = max(mu, T(1e-15)), r = max(theta, 1e-10), theta = theta_col[j],
                      else theta_row[row], else 0
    loss 4 (GP):      the KL weight 1 / max(mu, T(1e-4))
    loss 6, 7, 8:     min(1 / mu'^p, 1e6), p = 2, 3, power
    loss 0:           1 (only with robust > 0)
    robust > 0:       w *= 1 if |res sqrt(max(w, T(1e-15)))| <= robust else robust / (that + T(1e-15))
  G_w = G + sum (w - 1) f f^T  (+ l2 on the diagonal when l2 > 0);   b = sum f (w a) - G_w x_old
  x <- cd_maxit fixed CD sweeps on (G_w, b) from x_old, L1 inside the step, no L2 there (tests/cd_ref.py: cd_solve_batch)
  stop after the pass in which  max_i |x_i - x_old_i| / (|x_old_i| + T(1e-12)) < irls_tol
T(c) is the constant c rounded to the dtype of the kernel the result is compared with (`dtype`): the kernels and the reference
write these epsilons as Scalar(c).  Everything else runs in float64: for fp32 kernels this is a high-precision reference of the
same operation on the same (fp32-rounded) inputs, not a second fp32 computation -- in particular the weight, which the kernels
round to T, is not rounded here.
"""
import numpy as np

from tests.cd_ref import cd_solve_batch

W_CAP = 1e6


def _padded(A):
    """CSC (p, i, x) -> row indices, values and a validity mask, each (n, L), L = the longest column (at least 1)."""
    p = np.asarray(A.p, np.int64)
    n = len(p) - 1
    cnt = np.diff(p)
    L = max(int(cnt.max()) if n else 0, 1)
    pos = np.arange(L)[None, :]
    ok = pos < cnt[:, None]
    src = np.where(ok, p[:-1, None] + pos, 0)
    nnz = len(A.i)
    rows = np.where(ok, np.asarray(A.i, np.int64)[src] if nnz else 0, 0)
    vals = np.where(ok, np.asarray(A.x, np.float64)[src] if nnz else 0.0, 0.0)
    return rows, vals, ok


def irls_weight(loss_type, residual, mu, theta, power, robust, dtype):
    """The IRLS weight of every entry (arrays of one shape) and, with robust > 0, whether its Huber modifier is active."""
    T = np.dtype(dtype).type
    eps15, eps4 = float(T(1e-15)), float(T(1e-4))
    if loss_type == 0:
        w = np.ones_like(mu)
    elif loss_type == 4:
        w = 1.0 / np.maximum(mu, eps4)
    elif loss_type == 5:
        m = np.maximum(mu, eps15)
        r = np.maximum(theta, 1e-10)
        w = np.minimum(r / (m * (r + m)), W_CAP)
    elif loss_type in (6, 7, 8):
        m = np.maximum(mu, eps15)
        pw = {6: 2.0, 7: 3.0, 8: float(power)}[loss_type]
        with np.errstate(over="ignore", divide="ignore"):
            w = np.minimum(1.0 / np.power(m, pw), W_CAP)
    else:
        raise ValueError("loss_type")
    huber = np.zeros(np.shape(mu), bool)
    if robust > 0:
        ar = np.abs(residual * np.sqrt(np.maximum(w, eps15)))
        huber = ar > robust
        w = np.where(huber, w * (robust / (ar + eps15)), w)
    return w, huber


def irls_half_update(A, F, G, *, loss_type, dtype, l1=0.0, l2=0.0, nonneg=True, cd_maxit=100, irls_max_iter=5, irls_tol=1e-4,
                     theta_row=None, theta_col=None, power=1.5, robust=0.0, trace=None):
    """A: CSC holder (p, i, x; rows sorted or not), F: (rows, k), G: k x k base Gram; the scalar options as the kernel of `dtype`
    sees them (the caller rounds them).  All columns of a pass go at once: cd_solve_batch with one Gram per column.
    Returns (X (n, k), passes (n,), stat (n, irls_max_iter)): stat[j, p] = the stop statistic of pass p, NaN after the column's
    last pass.  trace (a dict, optional) receives  "X": the iterate after every pass (stopped columns carried forward),
    "w": the weights of every pass ((n, L) with "ok" the validity mask), "huber": the active Huber modifiers, "Gw": the weighted
    Gram of every column's last pass, "cancel" (n,): the worst cancellation of a reconstruction, sum |f_i x_i| / |f . x| over the
    passes and the entries whose weight depends on it."""
    T = np.dtype(dtype).type
    eps12 = float(T(1e-12))
    F = np.asarray(F, np.float64)
    G = np.asarray(G, np.float64)
    k = F.shape[1]
    rows, vals, ok = _padded(A)
    n = rows.shape[0]
    if theta_col is not None:
        theta = np.broadcast_to(np.asarray(theta_col, np.float64)[:, None], rows.shape)
    elif theta_row is not None:
        theta = np.asarray(theta_row, np.float64)[rows]
    else:
        theta = np.zeros(rows.shape)
    X = np.zeros((n, k))
    passes = np.full(n, irls_max_iter, np.int64)
    stat = np.full((n, max(irls_max_iter, 0)), np.nan)
    act = np.ones(n, bool)
    Gw_last = np.repeat(G[None], n, axis=0)
    if trace is not None:
        trace.update(X=[], w=[], huber=[], ok=ok, cancel=np.ones(n))
    for it in range(irls_max_iter):
        idx = np.nonzero(act)[0]
        if idx.size == 0:
            break
        Fr = F[rows[idx]]                                            # (na, L, k)
        xo = X[idx]
        mu = np.einsum("nlk,nk->nl", Fr, xo)
        w, hub = irls_weight(loss_type, vals[idx] - mu, mu, theta[idx], power, robust, dtype)
        dw = np.where(ok[idx], w - 1.0, 0.0)
        wa = np.where(ok[idx], w * vals[idx], 0.0)
        Gw = G[None] + np.einsum("nlr,nlc->nrc", Fr * dw[:, :, None], Fr)
        if l2 > 0:
            Gw[:, np.arange(k), np.arange(k)] += l2
        b = np.einsum("nlk,nl->nk", Fr, wa) - np.einsum("nrc,nc->nr", Gw, xo)
        xn = cd_solve_batch(Gw, b, xo, l1_cd=l1, nonneg=nonneg, maxit=cd_maxit, tol=0.0)[0]
        X[idx] = xn
        Gw_last[idx] = Gw
        rel = (np.abs(xn - xo) / (np.abs(xo) + eps12)).max(axis=1)
        stat[idx, it] = rel
        done = rel < irls_tol
        passes[idx[done]] = it + 1
        act[idx[done]] = False
        if trace is not None:
            # cancellation in the reconstructions: sum |f_i x_i| / mu, the factor by which a rounding error of the dot product grows
            # in mu and -- every weight but the capped ones being ~ 1 / mu^p -- in the weight; 1 when x >= 0
            can = np.einsum("nlk,nk->nl", np.abs(Fr), np.abs(xo)) / np.maximum(np.abs(mu), 1e-300)
            can = np.where(ok[idx] & (w < W_CAP) & (mu > 0), can, 1.0).max(axis=1)
            trace["cancel"][idx] = np.maximum(trace["cancel"][idx], can)
            wf = np.full(rows.shape, np.nan)
            wf[idx] = np.where(ok[idx], w, np.nan)
            hf = np.zeros(rows.shape, bool)
            hf[idx] = hub & ok[idx]
            trace["X"].append(X.copy()); trace["w"].append(wf); trace["huber"].append(hf)
    if trace is not None:
        trace["Gw"] = Gw_last
        while len(trace["X"]) < irls_max_iter:
            trace["X"].append(X.copy())
    return X, passes, stat
