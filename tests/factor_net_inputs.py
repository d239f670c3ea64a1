"""The inputs of the factor-graph parity tests, shared by tests/test_factor_net_cpu.py (which checks that the restatement's own
summation-order sensitivity `delta` stays at or under 1e-8 on every one of them) and tests/test_gpu_factor_net.py (which compares the
device with the restatement).  Pure numpy; the restatement's runs are cached and never modified.

delta: factor_net_ref.rel_diff between the restatement as written and its variant=True run (reversed visiting
order, long double accumulation), the largest over all outputs.  It never sees a device result.
"""
import functools
import os

import numpy as np

import factor_net_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
DELTA_MAX = 1e-8


def bound(delta):
    return 100 * max(delta, EPS)


@functools.lru_cache(maxsize=None)
def data(name):
    """(p, i, x, shape) or None, and the dense array."""
    if name == "hawaiibirds":
        z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
        shape = tuple(int(v) for v in z["shape"])
        p, i, x = z["p"].astype(np.int32), z["i"].astype(np.int32), z["x"].astype(np.float64)
        dense = np.zeros(shape)
        for j in range(shape[1]):
            dense[i[p[j]:p[j + 1]], j] = x[p[j]:p[j + 1]]
        return (p, i, x, shape), dense
    rng = np.random.default_rng(61)
    dense = rng.uniform(0, 1, (60, 40)) * (rng.uniform(size=(60, 40)) < 0.7)
    return None, dense


def cond_block(n, transposed=False):
    """A p = 2 condition block for n samples: two complementary group indicators; p x n, or n x p when transposed."""
    g = (np.arange(n) % 3 == 0).astype(np.float64)
    Z = np.stack([g, 1.0 - g])
    return Z.T.copy() if transposed else Z


def graph(name, n):
    """The restatement's graph (factor_net_ref.layer dicts) of a named topology over n samples."""
    L = F.layer
    if name == "chain":
        return [L(8), L(3, "layer", [0])]
    if name == "chain3":
        return [L(6), L(4, "layer", [0]), L(2, "layer", [1])]
    if name == "concat":
        return [L(5), L(3), L(4, "concat", [0, 1])]
    if name == "add":
        return [L(4), L(4), L(2, "add", [0, 1])]
    if name == "cond":
        return [L(8), L(3, "layer", [0], Z=cond_block(n))]
    if name == "cond_concat":
        return [L(5), L(3), L(4, "concat", [0, 1], Z=cond_block(n))]
    if name == "svd":
        return [L(8), L(3, "layer", [0], nonneg=(False, False))]
    if name == "penalties":
        return [L(8, L1=(0.0, 0.01)), L(3, "layer", [0], L2=(0.1, 0.0), ub=(0.0, 0.3))]
    if name == "small_chain":
        return [L(5), L(2, "layer", [0])]
    raise KeyError(name)


# (case name, data, topology, solver_mode, norm_type)
STEP_CASES = [
    ("chain-chol-L1", "hawaiibirds", "chain", 1, 0),
    ("chain-cd-L2", "hawaiibirds", "chain", 0, 1),
    ("concat-chol-none", "hawaiibirds", "concat", 1, 2),
    ("concat-cd-L1", "hawaiibirds", "concat", 0, 0),
    ("add-chol-L2", "hawaiibirds", "add", 1, 1),
    ("add-cd-L1", "hawaiibirds", "add", 0, 0),
    ("cond-chol-L1", "hawaiibirds", "cond", 1, 0),
    ("cond-concat-cd-L1", "hawaiibirds", "cond_concat", 0, 0),
    ("svd-chol-L1", "hawaiibirds", "svd", 1, 0),
    ("svd-cd-none", "hawaiibirds", "svd", 0, 2),
    ("penalties-chol-L1", "hawaiibirds", "penalties", 1, 0),
    ("penalties-cd-L2", "hawaiibirds", "penalties", 0, 1),
    ("dense-chol-L1", "dense", "small_chain", 1, 0),
    ("dense-cd-L1", "dense", "small_chain", 0, 0),
]
# (case name, data, topology, solver_mode, max_iter, tol)
FIT_CASES = [
    ("fit-chain-chol", "hawaiibirds", "chain", 1, 3, 1e-4),
    ("fit-concat-chol", "hawaiibirds", "concat", 1, 3, 1e-4),
    ("fit-chain-cd", "hawaiibirds", "chain", 0, 3, 1e-4),
    ("fit-chain-tol0.5", "hawaiibirds", "chain", 1, 20, 0.5),
]
SEED = 7


def layer_dims(g, m, n):
    dims = []
    for l in g:
        if l["kind"] == "input":
            dims.append((m, n))
            continue
        rows = dims[l["br"][0]][1]
        cols = g[l["br"][0]]["k"] if l["kind"] == "add" else sum(g[b]["k"] for b in l["br"])
        dims.append((rows, cols + (0 if l["Z"] is None else l["Z"].shape[0])))
    return dims


def start_states(g, m, n, seed):
    """Every layer's (W, d, H) for the start = 1 step tests: uniform (0.05, 1) factors, d = 1."""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0.05, 1.0, (r, l["k"])), np.ones(l["k"]), rng.uniform(0.05, 1.0, (l["k"], c)))
            for l, (r, c) in zip(g, layer_dims(g, m, n))]


def _delta(ref, var):
    return max(F.rel_diff(a, b) for a, b in zip(F.outputs(var), F.outputs(ref)))


@functools.lru_cache(maxsize=None)
def step_reference(case):
    """(graph, states, restatement result, delta) of a step case: one outer iteration from supplied states."""
    _, dname, topo, solver, norm = next(c for c in STEP_CASES if c[0] == case)
    dense = data(dname)[1]
    m, n = dense.shape
    g = graph(topo, n)
    states = start_states(g, m, n, 100 + [c[0] for c in STEP_CASES].index(case))
    kw = dict(max_iter=1, tol=0.0, solver=solver, norm=norm, states=states)
    ref = F.fit_deep(dense, g, **kw)
    return g, states, ref, _delta(ref, F.fit_deep(dense, g, variant=True, **kw))


@functools.lru_cache(maxsize=None)
def fit_reference(case):
    """(graph, restatement result, delta) of a full-fit case: warm-up and outer loop."""
    _, dname, topo, solver, max_iter, tol = next(c for c in FIT_CASES if c[0] == case)
    dense = data(dname)[1]
    g = graph(topo, dense.shape[1])
    kw = dict(max_iter=max_iter, tol=tol, seed=SEED, solver=solver, norm=0)
    ref = F.fit_deep(dense, g, **kw)
    return g, ref, _delta(ref, F.fit_deep(dense, g, variant=True, **kw))


def abi_graph(g):
    """The arguments of _abi.factor_net_fit after (csc, dense, m, n) for a restatement graph."""
    codes = {"input": 0, "layer": 1, "concat": 2, "add": 3}
    return dict(rank=[l["k"] for l in g], src_kind=[codes[l["kind"]] for l in g], branches=[l["br"] for l in g],
                cond_Z=[l["Z"] for l in g], L1=[l["L1"] for l in g], L2=[l["L2"] for l in g], upper_bound=[l["ub"] for l in g],
                nonneg=[l["nonneg"] for l in g])
