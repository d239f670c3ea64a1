"""numpy restatement of the reference's CPU deflation SVD with L21, angular and graph regularisation, with or without
cross-validation and an obs_mask -- the parity target of rcppml_gpu_svd_reg_ex / rcppml_gpu_svd_reg_dense_ex
(rcppml_amd/csrc/ops_svd.hip, kernels_svd_reg.hip.h).  Test infrastructure only: the product path never imports it.  With every new
term off it is svd_cv_ref.cv_deflation_svd, operation for operation.

Sources restated (reference tree, inst/include/FactorNet/svd/deflation.hpp), beside those of svd_cv_ref:
  :191-213   L21: L2_eff = L2 + L21 / |x| when |x| > 1e-10 (cast to the working precision), |x| before any shrinkage
  :256-267   angular: x -= (angular / nsq) F (F' x), F the k stored factors of the side; nothing at k = 0
  :283-292   graph: x -= (lambda / nsq) (L x), L as passed
  :734-742, :779-787   the order -- element chain, angular, graph -- on both sides of every iteration, nsq the CV-corrected
             |u_hat|^2 or |v|^2, before the normalisation

A graph is a COO triple (rows, cols, vals, dim), so that L x is the same sum in every dtype (np.longdouble included).
Also here: the parity cases of tests/test_gpu_svd_reg.py and MEASURED, the restatement's own float32-vs-float64 deviation on each.
Regenerate MEASURED with `python tests/svd_reg_ref.py`."""
import functools

import numpy as np

from rcppml_amd.data import splitmix64_uniform
from svd_cv_ref import effective_cv_seed, holdout_grid, planted
from svd_ref import regularize


# ------------------------------------------------------------------------------------------------ the three terms
def graph_matvec(g, x):
    """L x from the COO triple, entries added in the order given."""
    rows, cols, vals, dim = g
    out = np.zeros(dim, x.dtype)
    np.add.at(out, rows, vals.astype(x.dtype) * x[cols])
    return out


def l21_l2(x, L2, L21):
    """The L2 the element chain runs with (deflation.hpp:200-207)."""
    dt = x.dtype.type
    if L21 > 0:
        xn = np.sqrt(x @ x)
        if xn > dt(1e-10):
            return dt(L2) + dt(L21) / xn
    return L2


def angular_step(x, F, ang, nsq):
    """deflation.hpp:256-267; F: (len, k) stored factors."""
    if not ang > 0 or F.shape[1] == 0:
        return x
    dt = x.dtype.type
    return x - (dt(ang) / nsq) * (F @ (F.T @ x))


def graph_step(x, g, lam, nsq):
    """deflation.hpp:283-292."""
    if g is None or not lam > 0:
        return x
    dt = x.dtype.type
    return x - (dt(lam) / nsq) * graph_matvec(g, x)


def reg_side(x, F, nsq, L1, L2, nonneg, ub, L21, ang, g, lam):
    """One side's whole chain on the divided update x."""
    if L21 > 0:
        x = regularize(x, L1, l21_l2(x, L2, L21), nonneg, ub, nsq)
    else:
        x = regularize(x, L1, L2, nonneg, ub, nsq)
    x = angular_step(x, F, ang, nsq)
    return graph_step(x, g, lam, nsq)


# ------------------------------------------------------------------------------------------------ the loop
def reg_deflation_svd(A, k, stored=None, tol=1e-5, maxit=200, center=False, seed=0, L1=(0, 0), L2=(0, 0), nonneg=(False, False),
                      ub=(0, 0), L21=(0, 0), angular=(0, 0), graph_u=None, graph_v=None, graph_lambda=(0, 0), test_fraction=0.0,
                      cv_seed=0, patience=3, mask_zeros=False, obs_mask=None, dtype=np.float64):
    """svd_cv_ref.cv_deflation_svd with the three terms.  graph_u / graph_v: COO (rows, cols, vals, dim) or None.  Returns its dict
    plus dist: per factor, the 1 - |u . u_old| of every completed iteration."""
    A = np.asarray(A, np.float64)
    m, n = A.shape
    Ad = A.astype(dtype)
    mu = A.mean(axis=1).astype(dtype) if center else None
    frob = float(np.sum(A * A)) - (n * float(np.sum(A.mean(axis=1) ** 2)) if center else 0.0)
    eps100 = np.finfo(dtype).eps * 100
    rs = 42 if seed == 0 else int(seed)
    drawn = [0]
    do_cv = test_fraction > 0
    pattern = np.ones((m, n), bool) if stored is None else np.asarray(stored, bool)
    At = Ad.copy()
    n_masked = 0
    if obs_mask is not None:
        hit = np.asarray(obs_mask, bool) & pattern
        At[hit] = 0
        n_masked = int(hit.sum())
    rows = cols = np.zeros(0, np.int64)
    res = np.zeros(0, dtype)
    dc = dtype(1)
    if do_cv:
        held = holdout_grid(m, n, effective_cv_seed(seed, cv_seed), test_fraction) & pattern
        cols, rows = np.nonzero(held.T)
        res = Ad[rows, cols] - (mu[rows] if center else dtype(0))
        At[held] = 0
        nnz = int(pattern.sum())
        dens = dtype(nnz) / (dtype(m) * dtype(n))
        dc = dtype(1) - dtype(test_fraction) * (dens if mask_zeros else dtype(1))

    def rand_u():
        r = splitmix64_uniform(rs, drawn[0], m).astype(dtype)
        drawn[0] += m
        return r

    def at(u):
        y = At.T @ u
        return y - mu @ u if center else y

    def ax(v):
        y = At @ v
        return y - mu * v.sum() if center else y

    U = np.zeros((m, k), dtype)
    V = np.zeros((n, k), dtype)
    d = np.zeros(k, dtype)
    iters, losses, dist = [], [], []
    kcomp = best_k = waited = 0
    best = np.finfo(dtype).max
    by_patience = False
    for f in range(k):
        Uk, Vk, dk = U[:, :f], V[:, :f], d[:f]
        corr_v = lambda y, x: y - Vk @ (dk * (Uk.T @ x))
        corr_u = lambda y, x: y - Uk @ (dk * (Vk.T @ x))
        if f == 0:
            u = rand_u()
        else:
            u = U[:, f - 1].copy()
            for r in range(f):
                u = u - (u @ U[:, r]) * U[:, r]
            ni = np.sqrt(u @ u)
            if ni > eps100:
                u = u / ni
                v = corr_v(at(u), u)
                nv = np.sqrt(v @ v)
                if nv > 0:
                    v = v / nv
                u = corr_u(ax(v), v)
                for r in range(f):
                    u = u - (u @ U[:, r]) * U[:, r]
            else:
                u = rand_u()
        nu = np.sqrt(u @ u)
        if nu > 0:
            u = u / nu
        tol_k = dtype(tol)
        if f > 0 and d[0] > 0 and d[f - 1] > 0:
            tol_k = min(dtype(tol) * d[0] / d[f - 1], dtype(tol) * dtype(100))
        u_prev = u.copy()
        v = np.zeros(n, dtype)
        it = 0
        dist.append([])
        while it < maxit:
            u_old = u
            beta = dtype(it - 1) / dtype(it + 2) if it > 1 else dtype(0)
            uh = u + beta * (u - u_prev)
            u_prev = u
            usq = (uh @ uh) * dc
            if not usq > 0:
                v = np.zeros(n, dtype)
                break
            v = corr_v(at(uh), uh) / usq
            v = reg_side(v, Vk, usq, L1[1], L2[1], nonneg[1], ub[1], L21[1], angular[1], graph_v, graph_lambda[1])
            sv = np.sqrt(v @ v)
            if not sv > 0:
                break
            v = v / sv
            vsq = (v @ v) * dc
            u = corr_u(ax(v), v) / vsq
            u = reg_side(u, Uk, vsq, L1[0], L2[0], nonneg[0], ub[0], L21[0], angular[0], graph_u, graph_lambda[0])
            su = np.sqrt(u @ u)
            if not su > 0:
                break
            u = u / su
            dist[-1].append(1 - abs(u @ u_old))
            if dist[-1][-1] < tol_k:
                it += 1
                break
            it += 1
        if f > 0:
            for _ in range(2):
                u = u - Uk @ (Uk.T @ u)
            nn = np.sqrt(u @ u)
            if nn > eps100:
                u = u / nn
            for _ in range(2):
                v = v - Vk @ (Vk.T @ v)
            nn = np.sqrt(v @ v)
            if nn > eps100:
                v = v / nn
        sigma = abs(u @ corr_u(ax(v), v))
        U[:, f], V[:, f], d[f] = u, v, sigma
        iters.append(it)
        kcomp = f + 1
        if do_cv:
            res = res - sigma * u[rows] * v[cols]
            mse = (np.sum(res * res, dtype=dtype) / dtype(res.size)) if res.size else dtype(0)
            losses.append(mse)
            if mse < best:
                best, best_k, waited = mse, f + 1, 0
            else:
                waited += 1
                if waited >= patience:
                    by_patience = True
                    break
        else:
            best_k = f + 1
        if sigma < eps100:
            break
    return dict(u=U[:, :best_k], d=d[:best_k], v=V[:, :best_k], iters=np.array(iters), frob=frob,
                row_means=A.mean(axis=1) if center else None, k_selected=best_k, k_computed=kcomp,
                test_loss=np.array(losses, dtype), n_test=int(rows.size), n_masked=n_masked, stopped_by_patience=by_patience,
                rows=rows, cols=cols, dist=dist)


def deviation(got, ref):
    """The largest deviation of u, d and v, each relative to its largest reference magnitude (as svd_krylov_ref.deviation)."""
    out = 0.0
    for key in ("u", "d", "v"):
        b = np.asarray(ref[key], np.float64)
        if b.size:
            out = max(out, float(np.max(np.abs(np.asarray(got[key], np.float64) - b)) / max(np.max(np.abs(b)), 1e-300)))
    return out


# ------------------------------------------------------------------------------------------------ graphs
def ring_laplacian(dim, seed, skew=False):
    """COO of the weighted ring Laplacian: every vertex joined to its next two neighbours with weights in [0.5, 1.5); rows sum to
    zero.  skew: the upper-triangle weights are scaled by 0.7, which leaves a non-symmetric matrix (L x and L' x differ)."""
    rng = np.random.default_rng(seed)
    L = {}
    for step in (1, 2):
        w = 0.5 + rng.random(dim)
        for a in range(dim):
            b = (a + step) % dim
            if a == b:
                continue
            for i, j in ((a, b), (b, a)):
                wij = w[a] * (0.7 if skew and i < j else 1.0)
                L[(i, j)] = L.get((i, j), 0.0) - wij
                L[(i, i)] = L.get((i, i), 0.0) + wij
    keys = sorted(L, key=lambda ij: (ij[1], ij[0]))               # column-major, as a CSC stores it
    rows = np.array([ij[0] for ij in keys], np.int64)
    cols = np.array([ij[1] for ij in keys], np.int64)
    return rows, cols, np.array([L[ij] for ij in keys], np.float64), dim


def graph_dense(g):
    rows, cols, vals, dim = g
    L = np.zeros((dim, dim))
    L[rows, cols] = vals
    return L


def graph_csc(g, lam):
    """(p, i, x, dim, lambda) as _abi.svd_reg takes a graph (the COO is column-major already)."""
    rows, cols, vals, dim = g
    p = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=dim))]).astype(np.int32)
    return p, rows.astype(np.int32), vals.copy(), dim, float(lam)


def lambda_max_bound(g):
    """The largest absolute row sum of L: an upper bound of its spectral radius (exact to a few percent on these rings)."""
    rows, _, vals, dim = g
    return float(np.max(np.bincount(rows, weights=np.abs(vals), minlength=dim)))


# ------------------------------------------------------------------------------------------------ the parity cases
K, MAX_ITER = 5, 8
# close singular values: eight iterations leave every factor well short of convergence, so tol = 0 never meets a rounded distance
SIGMA = (12.0, 11.4, 10.8, 10.2, 9.6, 9.0, 8.4)
GRAPH_BUDGET = 0.05            # lambda * (bound of lambda_max(L)) on every graph of the table; the step misbehaves from about 0.4 on

SHAPES = {
    "dense65x63": (65, 63, None),
    "sparse130x67": (130, 67, 0.3),
    "sparse2100x70": (2100, 70, 0.1),
    "sparse70x2100": (70, 2100, 0.1),
}
PARAMS = {
    "l21": dict(L21=(0.3, 0.15)),
    "angular_nonneg": dict(angular=(0.2, 0.3), nonneg=(True, True)),
    "graph": dict(graphs="uv"),
    "graph_nonneg_center": dict(graphs="uv", skew=True, nonneg=(True, True), center=True),
    "all_l1_cv": dict(L21=(0.2, 0.1), angular=(0.2, 0.3), graphs="uv", L1=(0.01, 0.02), test_fraction=0.1),
    "all_mask": dict(L21=(0.2, 0.1), angular=(0.2, 0.3), graphs="uv", mask=True),
}
CASES = [(s, p) for s in SHAPES for p in PARAMS]
# fewer iterations where a factor of the restatement comes within 100 eps (float32) of convergence before MAX_ITER: at tol = 0 a
# rounded-negative distance would end the factor early in one precision and not in the other
ITERS = {("dense65x63", "angular_nonneg"): 5, ("dense65x63", "graph_nonneg_center"): 4, ("sparse130x67", "angular_nonneg"): 6,
         ("sparse130x67", "graph_nonneg_center"): 6}


def case_iters(shape, params):
    return ITERS.get((shape, params), MAX_ITER)


@functools.lru_cache(maxsize=None)
def shape_input(shape):
    """(A, stored pattern or None): planted close singular values, thinned for the sparse shapes; the 130 x 67 one has an empty row
    and an empty column."""
    m, n, dens = SHAPES[shape]
    A = planted(m, n, SIGMA, 3 + m, noise=0.05)
    if dens is None:
        return A, None
    keep = np.random.default_rng(7 + n).random(A.shape) < dens
    if shape == "sparse130x67":
        keep[7, :] = False
        keep[:, 3] = False
    return A * keep, keep


@functools.lru_cache(maxsize=None)
def shape_graphs(shape, skew):
    """(graph_u, graph_v, lambda_u, lambda_v): ring Laplacians with lambda * lambda_max_bound = GRAPH_BUDGET; skew: the u side's is
    non-symmetric."""
    m, n, _ = SHAPES[shape]
    gu, gv = ring_laplacian(m, 21, skew=skew), ring_laplacian(n, 22)
    return gu, gv, GRAPH_BUDGET / lambda_max_bound(gu), GRAPH_BUDGET / lambda_max_bound(gv)


def case_kwargs(shape, params):
    """(A, stored, keywords of reg_deflation_svd) of one case, tol = 0 and case_iters() iterations."""
    A, keep = shape_input(shape)
    kw = dict(PARAMS[params])
    out = dict(tol=0.0, maxit=case_iters(shape, params), seed=5)
    if kw.pop("graphs", None):
        gu, gv, lu, lv = shape_graphs(shape, bool(kw.pop("skew", False)))
        out.update(graph_u=gu, graph_v=gv, graph_lambda=(lu, lv))
    if kw.pop("mask", False):
        out["obs_mask"] = np.random.default_rng(31).random(A.shape) < 0.05
    out.update(kw)
    return A, keep, out


@functools.lru_cache(maxsize=None)
def case_ref(shape, params, dtype=np.float64):
    A, keep, kw = case_kwargs(shape, params)
    return reg_deflation_svd(A, K, stored=keep, dtype=dtype, **kw)


# the convergence cases (tol = 1e-5): one per precision, chosen so that at every factor's stopping iteration the distance is below
# tol_k / 2 and the one before above 2 tol_k in that precision's restatement (tests/test_svd_reg_cpu.py checks it)
CONVERGENCE = {
    np.float32: dict(shape="dense65x63", seed=53, params="all_mask"),
    np.float64: dict(shape="dense65x63", seed=66, params="all_mask"),
}
CONV_SIGMA = (40.0, 25, 12, 6, 3)


def convergence_kwargs(dtype):
    c = CONVERGENCE[dtype]
    m, n, dens = SHAPES[c["shape"]]
    A = np.abs(planted(m, n, CONV_SIGMA, 100 + c["seed"], noise=0.05))
    _, _, kw = case_kwargs(c["shape"], c["params"])
    kw = dict(kw, tol=1e-5, maxit=200)
    if dens is None:
        return A, None, kw
    keep = np.random.default_rng(200 + c["seed"]).random(A.shape) < dens
    return A * keep, keep, kw


def tol_k_of(d, f, tol, dtype):
    tk = dtype(tol)
    if f > 0 and d[0] > 0 and d[f - 1] > 0:
        tk = min(dtype(tol) * d[0] / d[f - 1], dtype(tol) * dtype(100))
    return tk


# The restatement's own float32-vs-float64 deviation on each case (deviation(): u, d, v), at case_iters() iterations and tol = 0.
# The fp32 device is held to four times these (tests/test_gpu_svd_reg.py).  Regenerate with `python tests/svd_reg_ref.py`.
MEASURED = {
    ('dense65x63', 'l21'): 2.62e-07,
    ('dense65x63', 'angular_nonneg'): 1.31e-07,
    ('dense65x63', 'graph'): 2.06e-07,
    ('dense65x63', 'graph_nonneg_center'): 3.00e-07,
    ('dense65x63', 'all_l1_cv'): 3.86e-07,
    ('dense65x63', 'all_mask'): 1.94e-07,
    ('sparse130x67', 'l21'): 1.25e-06,
    ('sparse130x67', 'angular_nonneg'): 6.34e-07,
    ('sparse130x67', 'graph'): 1.47e-06,
    ('sparse130x67', 'graph_nonneg_center'): 1.83e-07,
    ('sparse130x67', 'all_l1_cv'): 5.10e-07,
    ('sparse130x67', 'all_mask'): 5.23e-07,
    ('sparse2100x70', 'l21'): 1.79e-06,
    ('sparse2100x70', 'angular_nonneg'): 2.55e-06,
    ('sparse2100x70', 'graph'): 5.15e-06,
    ('sparse2100x70', 'graph_nonneg_center'): 1.78e-06,
    ('sparse2100x70', 'all_l1_cv'): 4.08e-06,
    ('sparse2100x70', 'all_mask'): 6.25e-07,
    ('sparse70x2100', 'l21'): 3.26e-07,
    ('sparse70x2100', 'angular_nonneg'): 3.85e-07,
    ('sparse70x2100', 'graph'): 3.75e-07,
    ('sparse70x2100', 'graph_nonneg_center'): 1.12e-06,
    ('sparse70x2100', 'all_l1_cv'): 4.81e-07,
    ('sparse70x2100', 'all_mask'): 4.03e-07,
}


if __name__ == "__main__":
    print("MEASURED = {")
    for s, p in CASES:
        dev = deviation(case_ref(s, p, np.float32), case_ref(s, p, np.float64))
        e = int(np.floor(np.log10(dev)))
        print("    (%r, %r): %.2fe%03d," % (s, p, np.ceil(dev / 10.0 ** e * 100) / 100, e))     # rounded up
    print("}")
