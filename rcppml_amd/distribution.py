"""Distribution diagnostics: host-side mirror of the reference R surface (R/auto_distribution.R) on the HIP path
(csrc/ops_distribution.hip).  score_test_distribution, diagnose_zero_inflation and diagnose_dispersion take mu = (W diag(d)) H from a
model (an NMFModel, or anything with .w (m x k), .d and .h (k x n)); the device forms mu a tile at a time and reduces it in the same
kernel, where R builds the dense m x n product.  auto_nmf_distribution fits each candidate loss with nmf() and compares information
criteria.  The decisions R takes on the host (labels, which.min, the modes, the cvs, AIC / BIC) are taken here with R's rules and
messages.  Input type decides the semantics as R's is_sparse does: scipy sparse input and CSC are sparse, a dense array is dense.
No CPU fallback: without a device the calls raise BackendError."""
import math

import numpy as np

from . import _abi
from . import nmf as _nmf
from ._abi import _check
from .data import CSC, as_matrix

POWER_LABELS = {"0": "gaussian", "1": "gp", "2": "gamma", "3": "inverse_gaussian"}
DISTRIBUTIONS = ("mse", "gp", "nb")
CRITERIA = ("bic", "aic")
_LOSS_POWER = {"mse": 0, "gaussian": 0, "gp": 1, "kl": 1, "gamma": 2, "inverse_gaussian": 3, "nb": 1}   # R's switch, default 0
NA_CONDITION = "missing value where TRUE/FALSE needed"


# ------------------------------------------------------------------------------------------------------------- R helpers
def _r_character(p):
    """as.character of a number (15 significant digits; whole numbers without a decimal point)."""
    p = float(p)
    if p.is_integer() and abs(p) < 1e15:
        return str(int(p))
    return "%.15g" % p


def power_label(p):
    s = _r_character(p)
    return POWER_LABELS.get(s, "power_" + s)


def which_min(v):
    """R's which.min: index of the first minimum, NaN skipped; None when nothing is left."""
    v = np.asarray(v, np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return None
    return int(np.flatnonzero(ok & (v == v[ok].min()))[0])


def _gt(a, b):
    """a > b in R's three-valued logic: None for NA."""
    return None if (math.isnan(a) or math.isnan(b)) else bool(a > b)


def _and(a, b):
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def _if(c):
    if c is None:
        raise ValueError(NA_CONDITION)
    return c


def _var(x):
    x = np.asarray(x, np.float64)
    return float(np.var(x, ddof=1)) if x.shape[0] > 1 else float("nan")


def _sd(x):
    return math.sqrt(_var(x)) if np.asarray(x).shape[0] > 1 else float("nan")


def _pmatch(a, choices):
    if a in choices:
        return a
    hits = [c for c in choices if a and c.startswith(a)]
    return hits[0] if len(hits) == 1 else None


def match_arg(arg, choices, several_ok=False):
    """R's match.arg(arg, choices, several.ok) with its messages ('arg' is the argument as R names it)."""
    if arg is None:
        return [choices[0]] if several_ok else choices[0]
    args = [arg] if isinstance(arg, str) else list(arg)
    if not several_ok:
        if tuple(args) == tuple(choices):
            return choices[0]
        if len(args) != 1:
            raise ValueError("'arg' must be of length 1")
    elif len(args) == 0:
        raise ValueError("'arg' must be of length >= 1")
    hits = [_pmatch(str(a), choices) for a in args]
    if all(h is None for h in hits):
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % c for c in choices))
    hits = [h for h in hits if h is not None]
    return hits if several_ok else hits[0]


# ------------------------------------------------------------------------------------------------------------ marshalling
def is_sparse(data):
    return isinstance(data, CSC) or hasattr(data, "tocsc")


def _matrix(data):
    """dict(csc=CSC or None, dense=column-major float64 or None, m, n)."""
    csc, dense = as_matrix(data)
    if csc is not None:
        return dict(csc=csc, dense=None, m=csc.rows, n=csc.cols)
    return dict(csc=None, dense=np.asfortranarray(dense), m=dense.shape[0], n=dense.shape[1])


def _model(model, m, n):
    """W_T as (m, k) row-major (= k x m), d (k), H as (n, k) row-major (= k x n)."""
    w = np.asarray(model.w, np.float64)
    d = np.asarray(model.d, np.float64).reshape(-1)
    h = np.asarray(model.h, np.float64)
    k = d.shape[0]
    if w.shape != (m, k) or h.shape != (k, n):
        raise ValueError("model dimensions (w %s, d %d, h %s) do not match the data (%d x %d)" % (w.shape, k, h.shape, m, n))
    return np.ascontiguousarray(w), np.ascontiguousarray(d), np.ascontiguousarray(h.T), k


# ------------------------------------------------------------------------------------------------------------ the four R functions
def score_test_distribution(data, model, powers=(0, 1, 2, 3), test_nb=True, min_mu=1e-6):
    """R's score_test_distribution: dict(scores (list of dict(power, T_stat, abs_T, distribution)), best_power, best_distribution,
    and nb_diagnostic = dict(T_NB, overdispersed) when test_nb and every observed x is integral).  The observed entries are the
    stored values != 0 for sparse data, all m*n for dense data."""
    M = _matrix(data)
    W_T, d, H, k = _model(model, M["m"], M["n"])
    powers = [float(p) for p in np.atleast_1d(np.asarray(powers, np.float64))]
    r = _check(_abi.score_test_double(M["csc"], M["dense"], M["m"], M["n"], k, W_T, d, H, powers, min_mu), "score test")
    scores = [dict(power=p, T_stat=float(t), abs_T=abs(float(t)), distribution=power_label(p)) for p, t in zip(powers, r["T"])]
    b = which_min([s["abs_T"] for s in scores])
    out = dict(scores=scores, best_power=None if b is None else scores[b]["power"],
               best_distribution=None if b is None else scores[b]["distribution"])
    if test_nb and r["all_integer"]:
        t = float(r["T_nb"])
        out["nb_diagnostic"] = dict(T_NB=t, overdispersed=_gt(t, 0.1))
    return out


def zi_mode(has_zi, row_excess, col_excess):
    """R's granularity rule (R/auto_distribution.R:342-356) in its three-valued logic."""
    if not has_zi:
        return "none"
    row_s = _gt(_var(row_excess), 0.001)
    col_s = _gt(_var(col_excess), 0.001)
    if _if(_and(row_s, col_s)):
        return "col"
    if _if(col_s):
        return "col"
    return "row"


def diagnose_zero_inflation(data, model, threshold=0.05):
    """R's diagnose_zero_inflation: dict(excess_zero_rate, has_zi, zi_mode, row_excess, col_excess).  Observed zeros of sparse
    data: m - stored entries per column, n - stored entries per row (a stored zero counts as a nonzero); of dense data: == 0."""
    M = _matrix(data)
    m, n = M["m"], M["n"]
    W_T, d, H, k = _model(model, m, n)
    r = _check(_abi.zero_inflation_double(M["csc"], M["dense"], m, n, k, W_T, d, H), "zero-inflation diagnostic")
    row_excess = np.maximum(0.0, (r["observed_row"] - r["expected_row"]) / n)
    col_excess = np.maximum(0.0, (r["observed_col"] - r["expected_col"]) / m)
    g = float(np.mean(np.concatenate([row_excess, col_excess])))
    has_zi = g > threshold
    return dict(excess_zero_rate=g, has_zi=has_zi, zi_mode=zi_mode(has_zi, row_excess, col_excess), row_excess=row_excess,
                col_excess=col_excess)


def loss_power(model):
    misc = getattr(model, "misc", None) or {}
    lt = misc.get("loss_type") or "mse"
    return _LOSS_POWER.get(lt, 0)


def dispersion_mode(row_cv, col_cv, cv_threshold):
    """R's mode rule (R/auto_distribution.R:436-445) in its three-valued logic."""
    r_s, c_s = _gt(row_cv, cv_threshold), _gt(col_cv, cv_threshold)
    if _if(_and(r_s, c_s)):
        return "per_row" if row_cv >= col_cv else "per_col"
    if _if(r_s):
        return "per_row"
    if _if(c_s):
        return "per_col"
    return "global"


def diagnose_dispersion(data, model, cv_threshold=0.5, min_mu=1e-6):
    """R's diagnose_dispersion: dict(mode, global_phi, row_cv, col_cv) plus row_phi and col_phi (R computes but does not return
    them).  phi = (x - mu')^2 / mu'^p over all m*n entries, p from model.misc["loss_type"]; trimmed means with trim 0.1."""
    M = _matrix(data)
    m, n = M["m"], M["n"]
    W_T, d, H, k = _model(model, m, n)
    r = _check(_abi.dispersion_double(M["csc"], M["dense"], m, n, k, W_T, d, H, float(loss_power(model)), min_mu, 0.1),
               "dispersion diagnostic")
    row_phi, col_phi = r["row_phi"], r["col_phi"]
    row_cv = _sd(row_phi) / float(np.mean(row_phi))
    col_cv = _sd(col_phi) / float(np.mean(col_phi))
    return dict(mode=dispersion_mode(row_cv, col_cv, cv_threshold), global_phi=r["global_phi"], row_cv=row_cv, col_cv=col_cv,
                row_phi=row_phi, col_phi=col_phi)


def information_criteria(dist, loss, k, m, n, N):
    """One comparison row: df, the NLL (mse: Gaussian NLL from the SSE), AIC and BIC (R/auto_distribution.R:91-115)."""
    df = k * (m + n) + 1 if dist == "mse" else k * (m + n) + m
    nll = (N / 2.0) * (1.0 + math.log(2.0 * math.pi * loss / N)) if dist == "mse" else float(loss)
    return dict(distribution=dist, nll=nll, df=df, aic=2.0 * nll + 2.0 * df, bic=2.0 * nll + df * math.log(N))


def auto_nmf_distribution(data, k, distributions=DISTRIBUTIONS, criterion=CRITERIA, maxit=50, seed=None, verbose=False, **kw):
    """R's auto_nmf_distribution: fit nmf(data, k, loss=dist, maxit, seed, verbose=False, ...) for each distribution, compare AIC /
    BIC.  Returns dict(loss, comparison (rows: distribution, nll, df, aic, bic, selected), models (by distribution))."""
    criterion = match_arg(criterion, CRITERIA)
    distributions = match_arg(distributions, DISTRIBUTIONS, several_ok=True)
    M = _matrix(data)
    m, n = M["m"], M["n"]
    N = int(np.count_nonzero(M["csc"].x)) if M["csc"] is not None else float(m) * n     # Matrix::nnzero
    models, rows = {}, []
    for dist in distributions:
        if verbose:
            print("Fitting NMF with loss = %s ..." % dist)
        model = _nmf.nmf(data, k, loss=dist, maxit=maxit, seed=seed, verbose=False, **kw)
        models[dist] = model
        rows.append(information_criteria(dist, model.misc["loss"], k, m, n, N))
    b = which_min([r[criterion] for r in rows])
    best = rows[b]["distribution"]
    for r in rows:
        r["selected"] = r["distribution"] == best
    if verbose:
        print("\n--- Distribution Comparison ( %s ) ---" % criterion.upper())
        print(" distribution          nll    df          aic          bic selected")
        for r in rows:
            print(" %12s %12.6g %5d %12.6g %12.6g %8s" % (r["distribution"], r["nll"], r["df"], r["aic"], r["bic"],
                                                         "TRUE" if r["selected"] else "FALSE"))
        print("\nBest distribution: %s " % best)
    return dict(loss=best, comparison=rows, models=models)
