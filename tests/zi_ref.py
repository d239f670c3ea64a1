"""Restatement of the reference's zero-inflated GP / NB fit (inst/include/FactorNet/nmf/fit_cpu.hpp) for the tests of nmf_zi().

Not product code.  The new pieces -- pi initialisation (:355-400), E-step (:1291-1437), M-step (:1439-1478) and soft imputation
(:1490-1550) -- are written as the reference's loops are: column by column, the rows of a column in order, the factor product
as a sum over the factors in order.  Everything else of the ALS loop (the IRLS half-updates, the Gram, the scaling, the dispersion
updates, the loss) is the oracle's.

Order of one ALS iteration as fit_cpu.hpp runs it (read at :444-1810):
  H half-update (:565-615)   iteration 0: nnls_batch_irls_sparse on A; later: nnls_batch_irls_dense on A_imputed
  extract_scaling(H) (:644)
  W half-update (:811-864)   iteration 0: sparse on A^T; later: dense on A_imputed^T
  extract_scaling(W_T) (:893)
  dispersion update (:914-1265) on the ORIGINAL A (GP theta / NB size)
  zi_em_iters x (E-step, M-step, theta floor) (:1285-1479) over the entries A does not store, with W_T diag(d) and H
  imputation (:1490-1550) from the original A and the updated pi
  loss (:1684-1767) on the original A's stored entries

Arrays follow the oracle: W_T is (m, k), H is (n, k) (memory = column-major k x m / k x n), A is an oracle Csc.
`acc` is the type of every accumulation (the factor product and the z sums); `reverse` visits columns, rows and factors in reverse.
The pair (float64, forward) / (longdouble, reverse) measures how much a summation order can move the result."""
import numpy as np

from oracle import oracle as O

GP, NB = 4, 5
ROW, COL, TWOWAY = 1, 2, 3


def stored_mask(A):
    """(m, n) bool: True where the CSC stores an entry (an explicit stored 0 included)."""
    S = np.zeros((A.rows, A.cols), bool)
    for j in range(A.cols):
        S[A.i[A.p[j]:A.p[j + 1]], j] = True
    return S


def pi_init(A, mode):
    """fit_cpu.hpp:355-400, sparse branch: pi = min(0.5 * (1 - stored / extent), 0.3)."""
    m, n = A.rows, A.cols
    if mode == ROW:
        cnt = np.zeros(m, np.int64)
        for j in range(n):
            for e in range(A.p[j], A.p[j + 1]):
                cnt[A.i[e]] += 1
        return np.array([min((1.0 - float(cnt[i]) / n) * 0.5, 0.3) for i in range(m)])
    cnt = np.diff(A.p).astype(np.int64)
    return np.array([min((1.0 - float(cnt[j]) / m) * 0.5, 0.3) for j in range(n)])


def s_entry(a_i, h_j, acc=np.float64, reverse=False):
    """max(sum_f a_i[f] h_j[f], 1e-10), the sum in factor order (:1328-1329)."""
    s = acc(0.0)
    order = range(len(a_i) - 1, -1, -1) if reverse else range(len(a_i))
    for f in order:
        s = s + acc(a_i[f]) * acc(h_j[f])
    return max(float(s), 1e-10)


def p0_entry(s, disp_i, loss):
    """P(Y = 0 | mu = s): NB (r / (r + s))^r with r = max(size, 1e-10) (:1333-1335); GP exp(-s / (1 + theta)) (:1337-1340)."""
    if loss == NB:
        r = max(float(disp_i), 1e-10)
        return float(np.power(r / (r + s), r))
    return float(np.exp(-s / (1.0 + float(disp_i))))


def z_entry(pi, p0):
    """:1356"""
    return pi / (pi + (1.0 - pi) * p0 + 1e-300)


def _s_column(a, h_j, rows, acc, reverse):
    """s of the given rows of one column: the factor sum in order, all rows at once."""
    s = np.zeros(len(rows), acc)
    k = a.shape[1]
    for f in (range(k - 1, -1, -1) if reverse else range(k)):
        s = s + a[rows, f].astype(acc) * acc(h_j[f])
    return np.maximum(s.astype(np.float64), 1e-10)


def _z_column(a, H, disp, pi, loss, mode, j, rows, acc, reverse):
    s = _s_column(a, H[j], rows, acc, reverse)
    if loss == NB:
        r = np.maximum(disp[rows], 1e-10)
        p0 = np.power(r / (r + s), r)
    else:
        p0 = np.exp(-s / (1.0 + disp[rows]))
    p = pi[rows] if mode == ROW else np.full(len(rows), pi[j])
    return p / (p + (1.0 - p) * p0 + 1e-300), s


def estep(A, W_T, d, H, disp, pi, loss, mode, acc=np.float64, reverse=False):
    """:1291-1437: (z_row_sum (m), z_col_sum (n), zero_count_row (m), zero_count_col (n)) over the entries A does not store."""
    m, n = A.rows, A.cols
    a = W_T * d[None, :]                          # apply_scaling (:1288-1289)
    S = stored_mask(A)
    zr, zc = np.zeros(m, acc), np.zeros(n, acc)
    cr, cc = np.zeros(m, np.int64), np.zeros(n, np.int64)
    for j in (range(n - 1, -1, -1) if reverse else range(n)):
        rows = np.nonzero(~S[:, j])[0]
        if reverse:
            rows = rows[::-1]
        if len(rows) == 0:
            continue
        z, _ = _z_column(a, H, disp, pi, loss, mode, j, rows, acc, reverse)
        loc = acc(0.0)
        for v in z:                               # z_col_local += z_ij, the rows in order
            loc = loc + acc(v)
        zc[j] = loc
        cc[j] = len(rows)
        zr[rows] = zr[rows] + z.astype(acc)       # z_row_local(i) += z_ij, the columns in order
        cr[rows] += 1
    return zr, zc, cr, cc


def mstep(pi, zr, zc, cr, cc, mode, m, n):
    """:1439-1470 (ROW / COL): clamp(zsum / extent, 0.001, 0.999) where the row / column has an unstored entry."""
    out = pi.copy()
    if mode == ROW:
        for i in range(m):
            if cr[i] > 0:
                out[i] = min(max(float(zr[i]) / float(n), 0.001), 0.999)
    else:
        for j in range(n):
            if cc[j] > 0:
                out[j] = min(max(float(zc[j]) / float(m), 0.001), 0.999)
    return out


def impute(A, W_T, d, H, disp, pi, loss, mode, acc=np.float64, reverse=False):
    """:1490-1550: A's stored values, z s elsewhere.  (m, n)."""
    m, n = A.rows, A.cols
    a = W_T * d[None, :]
    S = stored_mask(A)
    out = A.toarray()
    for j in range(n):
        rows = np.nonzero(~S[:, j])[0]
        if len(rows) == 0:
            continue
        z, s = _z_column(a, H, disp, pi, loss, mode, j, rows, acc, reverse)
        out[rows, j] = z * s
    return out


def zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters=1, theta_min=0.0, acc=np.float64, reverse=False):
    """The stage after the dispersion update: em_iters x (E, M, theta floor), then one imputation.  Returns (pi, disp, A_imputed)."""
    pi = np.asarray(pi, np.float64).copy()
    disp = np.asarray(disp, np.float64).copy()
    for _ in range(em_iters):
        zr, zc, cr, cc = estep(A, W_T, d, H, disp, pi, loss, mode, acc, reverse)
        pi = mstep(pi, zr, zc, cr, cc, mode, A.rows, A.cols)
        if loss == GP and theta_min > 0:          # :1473-1478 (theta_vec exists for GP only)
            disp = np.maximum(disp, theta_min)
    return pi, disp, impute(A, W_T, d, H, disp, pi, loss, mode, acc, reverse)


class ZiFit:
    pass


def zi_fit(A, W_T, H, loss=NB, mode=ROW, maxit=10, tol=0.0, em_iters=1, dispersion_mode=2, nb_size=(10.0, 1e6, 0.01),
           gp_theta=(0.1, 5.0, 0.0), L1=(0.0, 0.0), L2=(0.0, 0.0), nonneg=(True, True), cd_maxit=100, irls_max_iter=5,
           irls_tol=1e-4, norm_type=0, patience=5, sort_model=True, acc=np.float64, reverse=False):
    """The ALS loop of the module docstring, fp64.  L1 / L2 / nonneg are (W, H) pairs as in oracle.nmf_fit."""
    assert loss in (GP, NB) and mode in (ROW, COL) and dispersion_mode in (0, 1, 2)
    W_T = np.ascontiguousarray(W_T, np.float64).copy()
    H = np.ascontiguousarray(H, np.float64).copy()
    m, k = W_T.shape
    n = H.shape[0]
    d = np.ones(k)
    At = A.transpose()
    if loss == NB:
        disp = np.full(m, nb_size[1] if dispersion_mode == 0 else nb_size[0])
    else:
        disp = np.full(m, 0.0 if dispersion_mode == 0 else gp_theta[0])
    pi = pi_init(A, mode)
    pi0 = pi.copy()
    A_imp = A.toarray()
    th = disp if loss == NB else None
    prev, pat, hist = np.finfo(np.float64).max, 0, []
    r = ZiFit()
    r.converged, r.tol = False, 0.0
    for it in range(maxit):
        th = disp if loss == NB else None
        G = O.gram(W_T)
        if it == 0:
            H = O.irls(loss, A, W_T, G, k, L1[1], L2[1], nonneg[1], cd_maxit, irls_max_iter, irls_tol, theta_row=th)
        else:
            H = O.irls(loss, O.dense_as_csc(A_imp), W_T, G, k, L1[1], L2[1], nonneg[1], cd_maxit, irls_max_iter, irls_tol,
                       theta_row=th, dense_input=True)
        H, d = O.extract_scaling(H, norm_type)
        G = O.gram(H)
        if it == 0:
            W_T = O.irls(loss, At, H, G, k, L1[0], L2[0], nonneg[0], cd_maxit, irls_max_iter, irls_tol, theta_col=th)
        else:
            W_T = O.irls(loss, O.dense_as_csc(A_imp.T), H, G, k, L1[0], L2[0], nonneg[0], cd_maxit, irls_max_iter, irls_tol,
                         theta_col=th, dense_input=True)
        W_T, d = O.extract_scaling(W_T, norm_type)
        if dispersion_mode != 0:
            if loss == NB:
                disp = O.nb_size_update(A, W_T, H, d, disp, dispersion_mode, nb_size[2], nb_size[1])
            else:
                disp = O.dispersion_update(GP, A, W_T, H, d, disp, dispersion_mode, hi=gp_theta[1])
        pi, disp, A_imp = zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters, gp_theta[2], acc, reverse)
        lv = O.irls_loss(loss, A, W_T, d, H, disp)
        hist.append(lv)
        conv = False
        if it > 0:
            r.tol = abs(prev - lv) / (abs(prev) + 1e-15)
            conv = r.tol < tol
        prev = lv
        r.iter = it + 1
        if it > 0:
            if conv:
                pat += 1
                if pat >= patience:
                    r.converged = True
                    break
            else:
                pat = 0
    if sort_model:
        idx = np.argsort(-d, kind="stable")
        W_T, H, d = np.ascontiguousarray(W_T[:, idx]), np.ascontiguousarray(H[:, idx]), d[idx]
    r.W_T, r.H, r.d, r.theta, r.pi, r.pi_init, r.loss, r.loss_history, r.A_imputed = W_T, H, d, disp, pi, pi0, hist[-1], np.array(hist), A_imp
    return r


def simulate_zi_data(m=80, n=60, k=3, theta=0.5, dropout=0.2, seed=42):
    """The reference's tests/testthat/test_gpu_zi.R:16-30 with numpy generators (not R's streams): NB counts around W H with a
    Bernoulli dropout mask.  Returns an oracle Csc of the nonzero entries."""
    rng = np.random.default_rng(seed)
    W = np.abs(rng.normal(1, 0.5, (m, k)))
    W = W / W.sum(axis=0)[None, :]
    Hm = np.abs(rng.normal(1, 0.5, (k, n)))
    mu = W @ Hm
    size = np.maximum(mu / max(theta, 0.01), 0.1)
    Am = rng.negative_binomial(size, size / (size + mu)).astype(np.float64)
    if dropout > 0:
        Am = Am * rng.binomial(1, 1 - dropout, (m, n))
    return O.Csc.from_dense(Am)
