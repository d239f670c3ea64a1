"""Plain float64 numpy restatement of the reference's multi-layer factor-graph fit (inst/include/FactorNet/graph/fit.hpp:100-194
effective_input, :264-375 fit_deep), written from the C++ text; the tests compare the HIP path (rcppml_amd/csrc/ops_graph.hip) with
it.  The coordinate-descent solve is tests/cd_ref.py's.

graph:       a list of layers in topological order, each a dict
               k, kind ("input" | "layer" | "concat" | "add"), br (upstream layer indices), Z (p x rows or None),
               L1, L2, ub, nonneg: (W, H) pairs.
state:       per layer (W rows x k, d k, H k x cols).
input:       layer on the data: A (m x n, dense);  layer: t(H_up);  concat: [t(H_b1) | t(H_b2) | ...];  add: t(H_b1 + H_b2 + ...) in
             branch order;  a condition block appends t(Z).
iteration:   G = W^T W + 1e-15 I + L2_H I, B = W^T X, H = solve(G, B - L1_H) (CD from zero, or from the previous H with its residual
             correction when `warm`; Cholesky: the unconstrained solve, clipped), upper bound, H -> d (L1 / L2 / no norm, + 1e-15);
             G_saved = H H^T + 1e-15 I, the same for W on X^T with the W-side values (nmf/fit_cpu.hpp:486-893, the standard path of a
             dense input).
warm-up:     factors from one SplitMix64 stream seeded seed + i (W_T k x rows first, then H; nmf/nmf_init.hpp:166-182), then
             min(10, max_iter) iterations with the fit's convergence rule: the Gram-trick loss ||X||^2 - 2 cross + recon, relative
             change below tol on 5 consecutive checks (fit_cpu.hpp:1710-1807).
outer loop:  one cold iteration per layer in order, then every layer's mean squared reconstruction error summed; stop when
             |prev - cur| / (|prev| + 1e-15) < tol; total_loss is prev: the PREVIOUS iteration's loss when the loop stops on
             convergence, the last one when it runs out (fit.hpp:345-359).

variant=True is the same arithmetic with every contraction visited in reverse order and accumulated in np.longdouble, rounded to
double where the reference holds a double: the tests take the difference between the two as the scale of what a change of summation
order does to each output.
"""
import numpy as np

import cd_ref

LD = np.longdouble
EPS = 1e-15


def rel_diff(a, b):
    """max |a - b| / max(|a|, |b|) (0 when both are all zero): the measure of the parity tests."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.max(np.abs(b))) if b.size else 0.0, float(np.max(np.abs(a))) if a.size else 0.0)
    return 0.0 if scale == 0 else float(np.max(np.abs(a - b))) / scale


def _mm(X, Y, variant):
    """X @ Y; the variant contracts in reverse order in long double."""
    if not variant:
        return X @ Y
    return (np.ascontiguousarray(X[:, ::-1]).astype(LD) @ np.ascontiguousarray(Y[::-1, :]).astype(LD)).astype(np.float64)


def _mm_seq(X, Y, variant):
    """X @ Y with the contraction index visited in order, one rank-1 term at a time, in double: a plain sequential sum, whose
    rounding a blocked BLAS product would hide (a single k-term product against its own long-double value is what delta must see
    when the loss is one element).  The variant is _mm's."""
    if variant:
        return _mm(X, Y, True)
    P = np.zeros((X.shape[0], Y.shape[1]))
    for f in range(X.shape[1]):
        P += np.outer(X[:, f], Y[f])
    return P


def _rowsum(X, variant):
    if not variant:
        return X.sum(axis=1)
    return np.sum(X.astype(LD)[:, ::-1], axis=1).astype(np.float64)


def _total(X, variant):
    if not variant:
        return float(np.sum(X))
    return float(np.sum(X.astype(LD).ravel()[::-1]))


def splitmix_uniform(seed, offset, count):
    """uniform<double>() draws offset .. offset + count - 1 of SplitMix64(seed) (rng/rng.hpp:89-104)."""
    with np.errstate(over="ignore"):
        idx = np.arange(int(offset) + 1, int(offset) + int(count) + 1, dtype=np.uint64)
        z = np.uint64(int(seed)) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.astype(np.float64) / 2.0 ** 64


def init_factors(seed, k, rows, cols):
    """(W rows x k, H k x cols) of initialize_factors: one stream, W_T (k x rows, column-major) then H (k x cols, column-major)."""
    W = splitmix_uniform(seed, 0, k * rows).reshape(rows, k)
    H = splitmix_uniform(seed, k * rows, k * cols).reshape(cols, k).T
    return W.copy(), H.copy()


def layer(k, kind="input", br=(), Z=None, L1=(0.0, 0.0), L2=(0.0, 0.0), ub=(0.0, 0.0), nonneg=(True, True)):
    return dict(k=int(k), kind=kind, br=list(br), Z=None if Z is None else np.asarray(Z, np.float64), L1=tuple(L1), L2=tuple(L2),
                ub=tuple(ub), nonneg=tuple(nonneg))


def effective_input(i, graph, states, A):
    g = graph[i]
    if g["kind"] == "input":
        return A
    Hs = [states[b][2] for b in g["br"]]
    if g["kind"] == "add":
        S = Hs[0].copy()
        for Hb in Hs[1:]:
            S = S + Hb
        X = S.T
    else:
        X = np.concatenate([Hb.T for Hb in Hs], axis=1)
    if g["Z"] is not None:
        X = np.concatenate([X, g["Z"].T], axis=1)
    return np.ascontiguousarray(X)


def _solve(G, B, X0, l1, nonneg, ub, solver, warm, cd_maxit, cd_tol):
    """k x cols solution of one half-update; B k x cols, X0 the previous solution (read by a warm CD only)."""
    if solver == 1:
        X = np.linalg.solve(G, B - l1 if l1 > 0 else B)
        if nonneg:
            X = np.maximum(X, 0.0)
        if ub > 0:
            X = np.minimum(X, ub)
        return X
    X = cd_ref.cd_solve_batch(G, B.T, None if X0 is None else X0.T, l1_pre=l1, warm=warm, zero_init=not warm, nonneg=nonneg,
                              maxit=cd_maxit, tol=cd_tol, ub_post=ub)[0]
    return np.ascontiguousarray(X.T)


def _scale(X, norm, variant):
    """extract_scaling (nmf/variant_helpers.hpp:286-305): (X / d, d)."""
    k = X.shape[0]
    if norm == 2:
        return X, np.ones(k)
    d = _rowsum(np.abs(X), variant) if norm == 0 else np.sqrt(_rowsum(X * X, variant))
    d = d + EPS
    return X / d[:, None], d


def iterate(X, W, H, g, solver=1, norm=0, cd_maxit=100, cd_tol=1e-8, warm=False, variant=False, detail=None):
    """One iteration of the plain MSE fit of X ~ W diag(d) H from W (and, warm, from H): (W, d, H)."""
    k = g["k"]
    I = np.eye(k)
    Wt = np.ascontiguousarray(W.T)
    G = _mm(Wt, Wt.T, variant) + EPS * I + g["L2"][1] * I
    B = _mm(Wt, X, variant)
    H = _solve(G, B, H, g["L1"][1], g["nonneg"][1], g["ub"][1], solver, warm, cd_maxit, cd_tol)
    H, d = _scale(H, norm, variant)
    Gs = _mm(H, H.T, variant) + EPS * I
    Bw = _mm(H, np.ascontiguousarray(X.T), variant)
    Wt = _solve(Gs + g["L2"][0] * I, Bw, Wt, g["L1"][0], g["nonneg"][0], g["ub"][0], solver, warm, cd_maxit, cd_tol)
    Wt, d = _scale(Wt, norm, variant)
    if detail is not None:
        detail.update(Bw=Bw, Gs=Gs)
    return np.ascontiguousarray(Wt.T), d, H


def fit_loss(X, W, d, H, Bw, Gs, variant=False):
    """The fit's Gram-trick loss (fit_cpu.hpp:1710-1753) from the W update's raw right-hand side and saved Gram."""
    k = W.shape[1]
    tr = _total(X * X, variant)
    Wt = np.ascontiguousarray(W.T)
    Gwt = _mm(Wt, Wt.T, variant) + EPS * np.eye(k)
    cross = _total(d * _rowsum(Wt * Bw, variant), variant)
    recon = _total(np.outer(d, d) * Gwt * Gs, variant)
    return tr - 2.0 * cross + recon


def warm_up(X, g, seed, iters, tol, solver=1, norm=0, cd_maxit=100, cd_tol=1e-8, variant=False):
    """The warm-up fit of one layer: (W, d, H, iterations run)."""
    rows, cols = X.shape
    W, H = init_factors(seed, g["k"], rows, cols)
    d = np.ones(g["k"])
    prev, patience, ran = np.finfo(np.float64).max, 0, 0
    for it in range(iters):
        det = {}
        W, d, H = iterate(X, W, H, g, solver, norm, cd_maxit, cd_tol, warm=it > 0, variant=variant, detail=det)
        ran = it + 1
        loss = fit_loss(X, W, d, H, det["Bw"], det["Gs"], variant)
        conv = it > 0 and abs(prev - loss) / (abs(prev) + 1e-15) < tol
        prev = loss
        if it > 0:
            if conv:
                patience += 1
                if patience >= 5:
                    break
            else:
                patience = 0
    return W, d, H, ran


def layer_loss(X, W, d, H, variant=False):
    """||X - W diag(d) H||_F^2 / (rows cols) (fit.hpp:334-336)."""
    R = X - _mm_seq(W * d[None, :], H, variant)
    return _total(R * R, variant) / (X.shape[0] * X.shape[1])


def fit_deep(A, graph, max_iter=100, tol=1e-4, seed=0, solver=1, norm=0, cd_maxit=100, cd_tol=1e-8, states=None, variant=False):
    """dict(layers=[(W, d, H)], layer_loss, iter, converged, loss).  states: every layer's (W, d, H) -- the warm-up is skipped."""
    A = np.asarray(A, np.float64)
    seed_base = int(seed) if seed else 42
    kw = dict(solver=solver, norm=norm, cd_maxit=cd_maxit, cd_tol=cd_tol, variant=variant)
    if states is None:
        states = []
        for i, g in enumerate(graph):
            X = effective_input(i, graph, states, A)
            states.append(warm_up(X, g, (seed_base + i) & 0xFFFFFFFF, min(10, max_iter), tol, **kw)[:3])
    else:
        states = [tuple(np.array(v, np.float64) for v in s) for s in states]
    prev, total_iter, converged = np.inf, 0, False
    losses = [0.0] * len(graph)
    for _ in range(max_iter):
        for i, g in enumerate(graph):
            X = effective_input(i, graph, states, A)
            states[i] = iterate(X, states[i][0], states[i][2], g, warm=False, **kw)
        total_iter += 1
        losses = [layer_loss(effective_input(i, graph, states, A), *states[i], variant=variant) for i in range(len(graph))]
        cur = 0.0
        for v in losses:
            cur += v
        if np.isfinite(prev) and abs(prev - cur) / (abs(prev) + 1e-15) < tol:
            converged = True
            break
        prev = cur
    return dict(layers=states, layer_loss=np.asarray(losses), iter=total_iter, converged=converged, loss=prev)


def outputs(r):
    """Every array and number of a fit_deep result, for a delta over all outputs."""
    out = [r["layer_loss"], np.asarray([r["loss"]])]
    for W, d, H in r["layers"]:
        out += [W, d, H]
    return out
