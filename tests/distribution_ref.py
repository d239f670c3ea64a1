"""numpy restatement of the reference's R/auto_distribution.R for the tests: score_test_distribution (:194-266),
diagnose_zero_inflation (:304-366), diagnose_dispersion (:405-452) and the arithmetic of auto_nmf_distribution (:54-141).
Dense products, as R forms them.  Test infrastructure only: the package never imports this file."""
import math

import numpy as np

LABELS = {"0": "gaussian", "1": "gp", "2": "gamma", "3": "inverse_gaussian"}
NA_CONDITION = "missing value where TRUE/FALSE needed"


def parts(model):
    return np.asarray(model.w, np.float64), np.asarray(model.d, np.float64), np.asarray(model.h, np.float64)


def mu(model):
    """(W %*% diag(d)) %*% H"""
    w, d, h = parts(model)
    return (w * d[None, :]) @ h


def rpow(x, p):
    """R's x^p: x * x for p = 2, 1 for p = 0."""
    if p == 2:
        return x * x
    if p == 0:
        return np.ones_like(x)
    return np.power(x, p)


def csc_arrays(data):
    """(m, n, p, i, x) of a data.CSC or a scipy sparse matrix, or None for dense data."""
    if hasattr(data, "tocsc"):
        c = data.tocsc()
        c.sort_indices()
        return c.shape[0], c.shape[1], c.indptr, c.indices, c.data
    if hasattr(data, "p") and hasattr(data, "rows"):
        return data.rows, data.cols, data.p, data.i, data.x
    return None


def as_dense(data):
    s = csc_arrays(data)
    if s is None:
        return np.asarray(data, np.float64)
    m, n, p, i, x = s
    a = np.zeros((m, n))
    for j in range(n):
        a[i[p[j]:p[j + 1]], j] = x[p[j]:p[j + 1]]
    return a


def r_character(p):
    p = float(p)
    return str(int(p)) if p.is_integer() and abs(p) < 1e15 else "%.15g" % p


def label(p):
    s = r_character(p)
    return LABELS.get(s, "power_" + s)


def which_min(v):
    v = np.asarray(v, np.float64)
    best = None
    for q, a in enumerate(v):
        if not math.isnan(a) and (best is None or a < v[best]):
            best = q
    return best


def observed(data, model, min_mu):
    """x_obs, mu_obs: the stored entries with x != 0 (sparse) or all entries in column-major order (dense)."""
    M = mu(model)
    s = csc_arrays(data)
    if s is not None:
        m, n, p, i, x = s
        cols = np.repeat(np.arange(n), np.diff(p))
        keep = np.asarray(x) != 0
        xo = np.asarray(x, np.float64)[keep]
        mo = M[np.asarray(i)[keep], cols[keep]]
    else:
        xo = np.asarray(data, np.float64).ravel(order="F")
        mo = M.ravel(order="F")
    return xo, np.maximum(mo, min_mu)


def score_sums(data, model, powers, min_mu=1e-6):
    """sum(r^2 / mu'^p - 1) per power, sum((r^2 - mu') / mu'^2), count, all integral (math.fsum: close to exact)."""
    xo, mo = observed(data, model, min_mu)
    r = xo - mo
    r2 = r * r
    S = [math.fsum(r2 / rpow(mo, p) - 1.0) for p in powers]
    return S, math.fsum((r2 - mo) / (mo * mo)), xo.shape[0], bool(np.all(xo == np.round(xo)))


def score_test(data, model, powers=(0, 1, 2, 3), test_nb=True, min_mu=1e-6):
    S, snb, N, integral = score_sums(data, model, powers, min_mu)
    T = [s / N if N else float("nan") for s in S]
    scores = [dict(power=float(p), T_stat=t, abs_T=abs(t), distribution=label(p)) for p, t in zip(powers, T)]
    b = which_min([s["abs_T"] for s in scores])
    out = dict(scores=scores, best_power=None if b is None else scores[b]["power"],
               best_distribution=None if b is None else scores[b]["distribution"])
    if test_nb and integral:
        t = snb / N if N else float("nan")
        out["nb_diagnostic"] = dict(T_NB=t, overdispersed=None if math.isnan(t) else t > 0.1)
    return out


def zero_counts(data, model):
    """expected_row, expected_col, observed_row, observed_col."""
    E = np.exp(-np.maximum(mu(model), 1e-8))
    s = csc_arrays(data)
    if s is not None:
        m, n, p, i, x = s
        orow = n - np.bincount(np.asarray(i), minlength=m).astype(np.float64)
        ocol = m - np.diff(np.asarray(p)).astype(np.float64)
    else:
        a = np.asarray(data, np.float64)
        orow, ocol = (a == 0).sum(1).astype(np.float64), (a == 0).sum(0).astype(np.float64)
    return E.sum(1), E.sum(0), orow, ocol


def _var(x):
    return float(np.var(x, ddof=1)) if len(x) > 1 else float("nan")


def _gt(a, b):
    return None if (math.isnan(a) or math.isnan(b)) else a > b


def _and(a, b):
    if a is False or b is False:
        return False
    return None if (a is None or b is None) else True


def _if(c):
    if c is None:
        raise ValueError(NA_CONDITION)
    return c


def zi_mode(has_zi, row_excess, col_excess):
    if not has_zi:
        return "none"
    rs, cs = _gt(_var(row_excess), 0.001), _gt(_var(col_excess), 0.001)
    if _if(_and(rs, cs)):
        return "col"
    if _if(cs):
        return "col"
    return "row"


def zero_inflation(data, model, threshold=0.05):
    er, ec, orow, ocol = zero_counts(data, model)
    m, n = er.shape[0], ec.shape[0]
    row_excess = np.maximum(0.0, (orow - er) / n)
    col_excess = np.maximum(0.0, (ocol - ec) / m)
    g = float(np.mean(np.concatenate([row_excess, col_excess])))
    return dict(excess_zero_rate=g, has_zi=g > threshold, zi_mode=zi_mode(g > threshold, row_excess, col_excess),
                row_excess=row_excess, col_excess=col_excess)


POWERS = {"mse": 0, "gaussian": 0, "gp": 1, "kl": 1, "gamma": 2, "inverse_gaussian": 3, "nb": 1}


def phi(data, model, p, min_mu=1e-6):
    M = np.maximum(mu(model), min_mu)
    r = as_dense(data) - M
    return (r * r) / rpow(M, p)


def trim_bounds(N, trim=0.1):
    lo = int(math.floor(N * trim)) + 1
    return lo, N + 1 - lo


def trimmed_mean(x, trim=0.1):
    """R's mean(x, trim) for 0 <= trim < 0.5: the mean of the order statistics lo..hi (math.fsum: close to R's long double)."""
    x = np.sort(np.asarray(x, np.float64).ravel())
    N = x.shape[0]
    lo, hi = trim_bounds(N, trim)
    sel = x[lo - 1:hi]
    return math.fsum(sel) / sel.shape[0]


def dispersion_mode(row_cv, col_cv, t):
    rs, cs = _gt(row_cv, t), _gt(col_cv, t)
    if _if(_and(rs, cs)):
        return "per_row" if row_cv >= col_cv else "per_col"
    if _if(rs):
        return "per_row"
    if _if(cs):
        return "per_col"
    return "global"


def dispersion(data, model, cv_threshold=0.5, min_mu=1e-6):
    misc = getattr(model, "misc", None) or {}
    p = POWERS.get(misc.get("loss_type") or "mse", 0)
    P = phi(data, model, p, min_mu)
    row_phi = np.array([trimmed_mean(P[i, :]) for i in range(P.shape[0])])
    col_phi = np.array([trimmed_mean(P[:, j]) for j in range(P.shape[1])])
    sd = lambda v: math.sqrt(_var(v)) if len(v) > 1 else float("nan")   # noqa: E731
    row_cv = sd(row_phi) / float(np.mean(row_phi))
    col_cv = sd(col_phi) / float(np.mean(col_phi))
    return dict(mode=dispersion_mode(row_cv, col_cv, cv_threshold), global_phi=trimmed_mean(P), row_cv=row_cv, col_cv=col_cv,
                row_phi=row_phi, col_phi=col_phi)


def criteria(dist, loss, k, m, n, N):
    df = k * (m + n) + (1 if dist == "mse" else m)
    nll = (N / 2) * (1 + math.log(2 * math.pi * loss / N)) if dist == "mse" else loss
    return dict(distribution=dist, nll=nll, df=df, aic=2 * nll + 2 * df, bic=2 * nll + df * math.log(N))
