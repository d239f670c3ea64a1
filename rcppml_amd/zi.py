"""nmf_zi(): zero-inflated generalised-Poisson / negative-binomial NMF on the MI355X (rcppml_amd/csrc/ops_zi.hip).

The reference's nmf(..., loss = "gp" | "nb", zi = "row" | "col") (R/nmf_thin.R:227, :340-341, :358-360, :1300-1306), whose fit is
inst/include/FactorNet/nmf/fit_cpu.hpp:350-421, :589-596, :833-840, :1285-1552.  nmf(zi = ...) of this package still refuses (an existing
test pins that); this function is where the model is fitted, and routing nmf(zi = ...) to it is a later change.

Scope: fp64, sparse input (anything nmf() accepts is converted to a CSC: only the entries it stores count as observed, everything else
is a zero that may be structural), the CD solver, k <= 128, L1 / L2 / nonneg / upper_bound, dispersion none / global / per_row.  Masks,
cross-validation, fp32, graph / L21 / angular penalties, targets and the robust modifier are not offered under zero-inflation.
"""
import numpy as np

from . import _abi
from .data import r_runif, splitmix64_uniform
from .nmf import NMFModel, _as_csc, _pair, nmf

_ZI = ("none", "row", "col")


def nmf_zi(data, k, loss="nb", zi="row", zi_em_iters=1, tol=1e-4, maxit=100, L1=(0.0, 0.0), L2=(0.0, 0.0), seed=None,
           nonneg=(True, True), verbose=False, *, upper_bound=(0.0, 0.0), cd_maxit=100, cd_tol=1e-8, norm="L1", sort_model=True,
           patience=5, h_init=None, precision="fp64", dispersion="per_row", irls_max_iter=5, irls_tol=1e-4, nb_size_init=10.0,
           nb_size_max=1e6, nb_size_min=0.01, theta_init=0.1, theta_max=5.0, theta_min=0.0):
    """Zero-inflated NMF: A ~ w diag(d) h under loss "gp" or "nb" with a dropout probability per row (zi = "row") or per column
    (zi = "col"), estimated by EM beside the factors.  Arguments are nmf()'s; returns the same model object with misc["pi_row"] or
    misc["pi_col"] (and misc["theta"], the dispersion vector).

    From the second ALS iteration on, the entries the matrix does not store are replaced by z * mu (z the posterior dropout
    probability) and both half-updates weight every entry; the first iteration is the plain fit's.  `zi_em_iters`: E / M rounds per
    ALS iteration.  `zi = "none"` is nmf() itself.  Several seeds: one fit each, the lowest loss is returned (as nmf()).

    With the diagnostics:

        choice = auto_nmf_distribution(A, k)                    # {"loss": ..., "zi_mode": "none" | "row" | "col", ...}
        if choice["zi_mode"] != "none" and choice["loss"] in ("gp", "nb"):
            model = nmf_zi(A, k, loss=choice["loss"], zi=choice["zi_mode"])
    """
    if zi not in _ZI:
        raise ValueError("'arg' should be one of %s" % ", ".join(repr(x) for x in _ZI))          # match.arg(zi), R/nmf_thin.R:340
    kw = dict(tol=tol, maxit=maxit, L1=L1, L2=L2, nonneg=nonneg, verbose=verbose, upper_bound=upper_bound, cd_maxit=cd_maxit,
              cd_tol=cd_tol, norm=norm, sort_model=sort_model, patience=patience, h_init=h_init, precision=precision,
              dispersion=dispersion, irls_max_iter=irls_max_iter, irls_tol=irls_tol, nb_size_init=nb_size_init,
              nb_size_max=nb_size_max, nb_size_min=nb_size_min, theta_init=theta_init, theta_max=theta_max, theta_min=theta_min)
    if zi == "none":
        return nmf(data, k, loss=loss, seed=seed, **kw)
    if loss not in ("gp", "nb"):
        raise ValueError("zi != 'none' requires loss='gp' or loss='nb'.")                        # R/nmf_thin.R:358-360
    # ---- several initialisations: best of, one fit per seed (R/nmf_thin.R:744-786, :828-917)
    multi = None
    if isinstance(seed, (list, tuple)) and len(seed) > 0 and all(np.ndim(v) == 2 for v in seed):
        multi = list(seed)
    elif seed is not None and np.ndim(seed) == 1:
        multi = [int(v) for v in seed]
    if multi is not None and len(multi) > 1:
        fits = [nmf_zi(data, k, loss=loss, zi=zi, zi_em_iters=zi_em_iters, seed=sd, **kw) for sd in multi]
        losses = [f.misc["loss"] for f in fits]
        best = int(np.argmin(losses))
        fits[best].misc["all_init_losses"] = np.asarray(losses)
        fits[best].misc["best_init_idx"] = best
        return fits[best]
    if multi is not None:
        seed = multi[0]
    if precision != "fp64":
        raise NotImplementedError("zero-inflated losses run in fp64 on the MI355X backend (precision='fp64')")
    if dispersion not in ("none", "global", "per_row", "per_col"):
        raise ValueError("dispersion must be 'none', 'global', 'per_row' or 'per_col'")
    if dispersion == "per_col":
        raise NotImplementedError("zero-inflation with dispersion = 'per_col' is not implemented: the reference's E-step indexes the "
                                  "dispersion vector by row")
    if int(zi_em_iters) < 1:
        raise ValueError("'zi_em_iters' must be a positive integer")
    if not isinstance(sort_model, (bool, np.bool_)):
        raise ValueError("'sort_model' must be a single logical value")
    _nn = np.atleast_1d(np.asarray(nonneg))
    if _nn.dtype != np.bool_:
        raise ValueError("'nonneg' must be logical")
    if _nn.shape[0] not in (1, 2):
        raise ValueError("'nonneg' must be length 1 or 2 with no NA values")
    nnw, nnh = bool(_nn[0]), bool(_nn[-1])
    A = _as_csc(data)
    if np.isnan(A.x).any():
        raise ValueError("zero-inflated fits take no NA values (masks are not offered under zero-inflation)")
    m, n = A.shape
    k = int(k[0]) if np.ndim(k) == 1 else int(k)
    if k < 1:
        raise ValueError("k must be a positive integer")
    L1w, L1h = _pair(L1, "L1")
    L2w, L2h = _pair(L2, "L2")
    ubw, ubh = _pair(upper_bound, "upper_bound")
    if max(L1w, L1h) >= 1 or min(L1w, L1h) < 0:
        raise ValueError("L1 penalties must be strictly in the range [0,1)")
    if min(L2w, L2h) < 0:
        raise ValueError("L2 penalties must be strictly >= 0")
    if min(ubw, ubh) < 0:
        raise ValueError("'upper_bound' values must be non-negative")
    if norm not in ("L1", "L2", "none", "None"):
        raise ValueError("'arg' should be one of 'L1', 'L2', 'none'")
    norm_type = {"L1": 0, "L2": 1, "none": 2, "None": 2}[norm]
    # ---- initialisation, as nmf()
    if seed is None:
        seed_int = int(np.random.SeedSequence().generate_state(1)[0] % (2 ** 31 - 1)) + 1
        W0 = r_runif(seed_int, m * k).reshape(k, m).T.copy()
    elif np.ndim(seed) == 2:
        s = np.asarray(seed, dtype=np.float64)
        if s.shape == (m, k):
            W0 = s.copy()
        elif s.shape == (k, m):
            W0 = s.T.copy()
        else:
            raise ValueError("Custom init matrix dimensions incompatible with data")
        seed_int = int(abs(int(np.sum(s * 1e6) % (2 ** 31 - 1))))
    else:
        seed_int = int(seed)
        W0 = r_runif(seed_int, m * k).reshape(k, m).T.copy()
    W_T = np.ascontiguousarray(W0, dtype=np.float64)
    if h_init is not None:
        H = np.ascontiguousarray(np.asarray(h_init, dtype=np.float64).T)
        if H.shape != (n, k):
            raise ValueError("h_init must be k x n")
    else:
        H = splitmix64_uniform(seed_int & 0xFFFFFFFF, 0, k * n, np.float64).astype(np.float64).reshape(n, k)
    res = _abi.nmf_zi_double(A.p, A.i, A.x, m, n, k, W_T, H, zi_mode=_abi.ZI_MODE[zi], zi_em_iters=int(zi_em_iters),
                             loss_type={"gp": 4, "nb": 5}[loss], max_iter=int(maxit), tol=float(tol), L1_H=L1h, L1_W=L1w, L2_H=L2h,
                             L2_W=L2w, ub_H=ubh, ub_W=ubw, cd_maxit=int(cd_maxit), cd_tol=float(cd_tol), verbose=int(verbose),
                             patience=int(patience), nonneg_W=int(nnw), nonneg_H=int(nnh), irls_max_iter=int(irls_max_iter),
                             irls_tol=float(irls_tol), norm_type=norm_type,
                             dispersion_mode={"none": 0, "global": 1, "per_row": 2}[dispersion],
                             gp_theta=(float(theta_init), float(theta_max), float(theta_min)),
                             nb_size=(nb_size_init, nb_size_max, nb_size_min), sort_model=int(sort_model))
    if res["status"] != 0:
        raise _abi.BackendError("GPU zero-inflated NMF failed: %s" % res.get("error"))
    misc = dict(tol=res["tol"], iter=res["iter"], loss=res["loss"], loss_history=res.get("loss_history"), converged=res["converged"],
                solver="cd", solver_mode=0, L1=(L1w, L1h), L2=(L2w, L2h), seed=seed_int, precision=precision, resource="gpu",
                loss_type=loss, zi=zi, zi_em_iters=int(zi_em_iters), theta=res["theta"], entry="rcppml_gpu_nmf_zi_double")
    misc["pi_row" if zi == "row" else "pi_col"] = res["pi"]                              # R/nmf_thin.R:1300-1306
    return NMFModel(w=W_T.copy(), d=res["d"].copy(), h=H.T.copy(), misc=misc)
