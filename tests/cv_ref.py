"""Plain numpy restatement of the cross-validation half-updates and losses -- the parity target of rcppml_hip_solve_cv,
rcppml_hip_solve_cv_irls, rcppml_hip_cv_test_error and rcppml_hip_cv_irls_loss.  Test infrastructure only: no torch, no GPU code,
no oracle; tests/test_cv_ref_cpu.py pins it to the oracle (fp64), the GPU tests compare every kernel with it.

Semantics restated from the reference's rules as oracle/nmf_oracle.cpp cites them (nmf/speckled_cv.hpp:57-83, rng/rng.hpp:129-170,
nmf/cv_detail.hpp:66-85, :101-292, :304-505, nmf/fit_cv.hpp:420-830, :1377-1494):

  hold-out mask    entry (i, j) of A -- always A's coordinates, also on the W side -- is held out when
                   hash(seed, i, j) < UINT64_MAX // inv_prob, hash = SplitMix64's finaliser of seed + i c1 + j c2,
                   seed = (uint32) cv_seed with 0 -> 12345, inv_prob = (uint64)(1 / fraction).  The truncation is the reference's:
                   0.34 holds out one half, anything above 0.5 every entry.
  MSE half-update  per column j of D (D = A and F = W on the H side, D = A^T and F = H on the W side):
                   b = sum over the training nonzeros a f_row;  G_local = G - sum f f^T over the held-out rows (mask_zeros: the
                   held-out NONZEROS only);  a user-masked row that is not already one of those rows leaves b and joins them;
                   x = clip(G_local^-1 (b - L1)) (Cholesky) or cd_maxit coordinate sweeps with L1 inside the step, started
                   from the current column, b NOT corrected for the start.
  IRLS half-update per column, up to irls_max_iter passes over the training entries (mask_zeros: the nonzeros that are neither
                   held out nor user-masked; else every such row, zeros included):  mu = f . x,  w = weight(a - mu, mu) with
                   observed = 0 and theta = 0 (GP: irls_weight_gp, not the KL weight), Huber modifier when robust > 0, cap 1e6;
                   G_w = sum w f f^T + G_add + T(1e-15) I from zero every pass;  b_w = sum (w a) f, no residual correction;
                   the same two solves;  stop after the pass with  max_i |x_i - xold_i| / (|xold_i| + T(1e-12)) < irls_tol.
  held-out error   sum of (a - (w_i d) . h_j)^2 and count over the held-out entries (mask_zeros: held-out nonzeros).
  losses           per-element loss summed separately over training and held-out entries, with counts; user-masked entries
                   are in neither; GP takes theta of the entry's row, every other loss theta = 0.
T(c) is the constant c rounded to the dtype of the kernel compared (`dtype`); W d is rounded to that dtype too (the reference
holds it as a Scalar matrix).  Everything else runs in `xp`: float64 -- a high-precision reference of the same operation on the
same dtype-rounded inputs -- or numpy.longdouble, against which the fp64 oracle's own rounding is measured."""
import numpy as np

U64 = (1 << 64) - 1
W_CAP = 1e6


def cv_hash(seed, i, j):
    """SplitMix64::hash(seed, i, j) on broadcast integer arrays -> uint64 (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        h = (np.uint64(seed & U64) + np.asarray(i).astype(np.uint64) * np.uint64(0x9e3779b97f4a7c15)
             + np.asarray(j).astype(np.uint64) * np.uint64(0x6c62272e07bb0142))
        h = (h ^ (h >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return h ^ (h >> np.uint64(31))


def mask_params(fraction, cv_seed):
    """(seed, threshold) as Python integers."""
    s32 = int(cv_seed) & 0xFFFFFFFF
    inv_prob = int(1.0 / fraction)
    return (12345 if s32 == 0 else s32), U64 // inv_prob


def holdout(rows, cols, fraction, cv_seed):
    """Boolean rows x cols, A's coordinates."""
    seed, thr = mask_params(fraction, cv_seed)
    return cv_hash(seed, np.arange(rows)[:, None], np.arange(cols)[None, :]) < np.uint64(thr)


def dense(D, xp=np.float64):
    """CSC holder (rows, cols, p, i, x) -> (stored (rows x cols, bool), values (rows x cols, xp))."""
    S = np.zeros((D.rows, D.cols), bool)
    V = np.zeros((D.rows, D.cols), xp)
    cols_of = np.repeat(np.arange(D.cols), np.diff(D.p))
    S[D.i, cols_of] = True
    if getattr(D, "x", None) is not None and len(D.x) == len(D.i):
        V[D.i, cols_of] = np.asarray(D.x).astype(xp)
    return S, V


def chol_solve_batch(G, B):
    """x = G^-1 b for every (G[n], B[n]) through the lower Cholesky factor, in the dtype of G."""
    n, k, _ = G.shape
    L = np.zeros_like(G)
    for c in range(k):
        s = G[:, c:, c] - np.einsum("nip,np->ni", L[:, c:, :c], L[:, c, :c])
        L[:, c:, c] = s / np.sqrt(s[:, :1])
    y = np.zeros_like(B)
    for i in range(k):
        y[:, i] = (B[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
    x = np.zeros_like(B)
    for i in range(k - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x


def cd_fixed_batch(G, B, X0, l1, nonneg, maxit):
    """cd_nnls_col_fixed on every (G[n], B[n], X0[n]): maxit sweeps in coordinate order, step b_i / g_ii - l1, clamp at 0 when
    nonneg, b -= step g_i; no tolerance, no warm-start correction (tests/cd_ref.py: cd_solve_batch with tol = 0, any dtype)."""
    B, X = B.copy(), X0.copy()
    k = B.shape[1]
    for _ in range(maxit):
        for i in range(k):
            g = G[:, i, i]
            ok = g > 0
            xi = X[:, i]
            diff = B[:, i] / np.where(ok, g, 1)
            if l1 != 0:
                diff = diff - l1
            nv = xi + diff
            a, nx = diff, nv
            if nonneg:
                neg = nv < 0
                a = np.where(neg, -xi, a)
                nx = np.where(neg, 0, nx)
            a = np.where(ok, a, 0)
            X[:, i] = np.where(ok, nx, xi)
            B -= a[:, None] * G[:, i]
    return X


def weighted_grams(Wt, F):
    """sum_r Wt[n, r] f_r f_r^T for every n, as one matrix product: (n, rows) @ (rows, k k)."""
    k = F.shape[1]
    return (Wt @ (F[:, :, None] * F[:, None, :]).reshape(F.shape[0], k * k)).reshape(Wt.shape[0], k, k)


def _solve(Gl, b, x0, l1, nonneg, cd_maxit, solver_mode):
    if solver_mode == 1:
        x = chol_solve_batch(Gl, b - l1 if l1 > 0 else b)
        return np.maximum(x, 0) if nonneg else x
    return cd_fixed_batch(Gl, b, x0, l1, nonneg, cd_maxit)


def mse_half_update(D, F, G, X0, held, *, mask_zeros, umask=None, l1=0.0, nonneg=True, cd_maxit=100, solver_mode=0, xp=np.float64,
                    trace=None):
    """D: CSC holder; F (D.rows, k); G k x k; X0 (D.cols, k); held: boolean D.rows x D.cols (the hold-out mask in D's orientation);
    umask: the user mask in D's orientation (boolean, or None).  trace (dict) receives "Gl", the per-column Gram."""
    S, V = dense(D, xp)
    F, G, X0 = np.asarray(F).astype(xp), np.asarray(G).astype(xp), np.asarray(X0).astype(xp)
    U = np.zeros_like(S) if umask is None else umask
    test = held & S if mask_zeros else held
    corr = (test | U).T.astype(xp)                                     # (cols, rows): rows out of the column's Gram
    train = (S & ~held & ~U).T
    b = np.where(train, V.T, 0) @ F
    Gl = G[None] - weighted_grams(corr, F)
    if trace is not None:
        trace["Gl"] = Gl
    return _solve(Gl, b, X0, xp(l1), nonneg, cd_maxit, solver_mode)


def cv_irls_weight(loss_type, residual, mu, power, robust, dtype):
    """compute_irls_weight(residual, predicted) with observed = 0 and theta = 0.  Returns (w, capped, huber)."""
    T = np.dtype(dtype).type
    eps15 = float(T(1e-15))
    xp = mu.dtype.type
    m = np.maximum(mu, xp(eps15))
    with np.errstate(over="ignore", divide="ignore"):
        if loss_type == 0:
            raw = np.ones_like(mu)
        elif loss_type == 4:                                           # irls_weight_gp(0, mu, 0, blend = 1)
            eb = np.minimum(m, 1)
            w_gp = 1 / (m * m)
            blend = np.exp((1 - eb) * -np.log(m) + eb * np.log(np.maximum(w_gp, xp(1e-300))))
            raw = np.where(eb < 0.999, blend, w_gp)
        elif loss_type == 5:
            r = xp(1e-10)
            raw = r / (m * (r + m))
        elif loss_type in (6, 7, 8):
            raw = 1 / np.power(m, xp({6: 2.0, 7: 3.0, 8: float(power)}[loss_type]))
        else:
            raise ValueError("loss_type")
    capped = raw > W_CAP
    w = np.where(capped, xp(W_CAP), raw) if loss_type != 0 else raw
    huber = np.zeros(mu.shape, bool)
    if robust > 0:
        ar = np.abs(residual * np.sqrt(np.maximum(w, xp(eps15))))
        huber = ar > robust
        w = np.where(huber, w * (xp(robust) / (ar + xp(eps15))), w)
    return w, capped, huber


def irls_half_update(D, F, G_add, X0, held, *, mask_zeros, loss_type, dtype, umask=None, l1=0.0, nonneg=True, cd_maxit=100,
                     solver_mode=0, irls_max_iter=5, irls_tol=1e-4, power=1.5, robust=0.0, xp=np.float64, trace=None):
    """Arguments as in mse_half_update; the scalar options as the kernel of `dtype` sees them (the caller rounds them).
    Returns (X, passes (cols,), stat (cols, irls_max_iter): the stop statistic of every pass, NaN after the column's last).
    trace (dict) receives "capped" / "huber": whether any training weight sat at the cap / had an active Huber modifier."""
    T = np.dtype(dtype).type
    eps15, eps12 = xp(float(T(1e-15))), xp(float(T(1e-12)))
    S, V = dense(D, xp)
    F, X = np.asarray(F).astype(xp), np.asarray(X0).astype(xp).copy()
    k = F.shape[1]
    Ga = np.zeros((k, k), xp) if G_add is None else np.asarray(G_add).astype(xp)
    U = np.zeros_like(S) if umask is None else umask
    train = ((S if mask_zeros else np.ones_like(S)) & ~held & ~U).T     # (cols, rows)
    Vt = V.T
    n = D.cols
    passes = np.full(n, irls_max_iter, np.int64)
    stat = np.full((n, max(irls_max_iter, 0)), np.nan)
    act = np.ones(n, bool)
    if trace is not None:
        trace.update(capped=False, huber=False, below_cap=False)
    for it in range(irls_max_iter):
        idx = np.nonzero(act)[0]
        if idx.size == 0:
            break
        xo = X[idx]
        mu = xo @ F.T
        w, capped, huber = cv_irls_weight(loss_type, Vt[idx] - mu, mu, power, robust, dtype)
        w = np.where(train[idx], w, 0)
        Gw = weighted_grams(w, F) + Ga[None]
        Gw[:, np.arange(k), np.arange(k)] += eps15
        bw = (w * Vt[idx]) @ F
        xn = _solve(Gw, bw, xo, xp(l1), nonneg, cd_maxit, solver_mode)
        X[idx] = xn
        rel = (np.abs(xn - xo) / (np.abs(xo) + eps12)).max(axis=1)
        stat[idx, it] = rel
        done = rel < irls_tol
        passes[idx[done]] = it + 1
        act[idx[done]] = False
        if trace is not None:
            trace["capped"] |= bool((capped & train[idx]).any())
            trace["below_cap"] |= bool((~capped & train[idx]).any())
            trace["huber"] |= bool((huber & train[idx]).any())
    return X, passes, stat


def _predictions(W, d, H, dtype, xp):
    Wd = (np.asarray(W, dtype) * np.asarray(d, dtype)[None, :]).astype(xp)                 # a Scalar matrix in the reference
    return Wd @ np.asarray(H, dtype).astype(xp).T                                           # (rows, cols)


def heldout_error(A, W, d, H, held, *, mask_zeros, dtype, xp=np.float64):
    """(sum of squared held-out errors, their count); held in A's coordinates."""
    S, V = dense(A, xp)
    use = held & S if mask_zeros else held
    diff = V - _predictions(W, d, H, dtype, xp)
    return float((diff * diff)[use].sum()), int(use.sum())



def loss_terms(loss_type, y, mu, theta, power):
    """loss_contribution of math/loss.hpp:382-505 (loss_type 0: squared error), elementwise in the dtype of mu."""
    xp = mu.dtype.type
    if loss_type == 0:
        return (y - mu) * (y - mu)
    m = np.maximum(mu, xp(1e-10))
    if loss_type == 4:
        opt = 1 + theta
        inner = np.maximum((m + theta * y) / opt, xp(1e-10))
        return -np.log(m / opt) - np.where(y >= 1, (y - 1) * np.log(inner), 0) + (m + theta * y) / opt
    if loss_type == 5:
        from scipy.special import gammaln
        r = xp(1e-10)                                                   # theta = 0, floored
        lg = (gammaln(np.full(y.shape, float(r))) - gammaln(y.astype(np.float64) + float(r))).astype(mu.dtype)
        return lg - r * np.log(r / (r + m)) - y * np.log(m / (r + m))
    yy = np.maximum(y, xp(1e-10))
    pp = {6: 2.0, 7: 3.0, 8: float(power)}[loss_type]
    if loss_type == 7:
        return (yy - m) ** 2 / (m * m * yy)
    if abs(pp - 1.0) < 1e-6:
        return 2 * (yy * np.log(yy / m) - (yy - m))
    if abs(pp - 2.0) < 1e-6:
        return 2 * (-np.log(yy / m) + (yy - m) / m)
    omp, tmp = xp(1.0 - pp), xp(2.0 - pp)
    return 2 * (np.power(yy, tmp) / (omp * tmp) - yy * np.power(m, omp) / omp + np.power(m, tmp) / tmp)


def explicit_loss(A, W, d, H, held, *, mask_zeros, loss_type, dtype, theta=None, power=1.5, umask=None, xp=np.float64):
    """(train sum, n_train, test sum, n_test); held and umask in A's coordinates; theta per row of A (GP only)."""
    S, V = dense(A, xp)
    use = S.copy() if mask_zeros else np.ones_like(S)
    if umask is not None:
        use &= ~umask
    th = np.zeros((A.rows, 1), xp)
    if loss_type == 4 and theta is not None:
        th = np.asarray(theta, dtype).astype(xp)[:, None]
    lv = loss_terms(loss_type, V, _predictions(W, d, H, dtype, xp), np.broadcast_to(th, V.shape), power)
    tr, te = use & ~held, use & held
    return float(lv[tr].sum()), int(tr.sum()), float(lv[te].sum()), int(te.sum())
