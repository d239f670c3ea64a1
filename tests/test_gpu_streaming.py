"""GPU checks of the panel-streamed fit (csrc/ops_stream.hip): the two W-side sums against numpy float64 on
panels placed on the row-tile boundaries of rcppml_hip_stream_geometry, their repeatability, nmf_streaming() against nmf(), and the
refusals.  Bounds follow DESIGN.md section 7: delta = max|a - b| / max|b| of the resident op (rcppml_hip_rhs on the transpose,
rcppml_hip_gram; or nmf() against the float64 oracle fit) from the float64 answer, and the streamed path gets 100 * max(delta, 2^-52)."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import oracle as O
from rcppml_amd import _abi, nmf_streaming
from rcppml_amd.nmf import nmf
from rcppml_amd.data import CSC, simulate_nmf_sparse

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp32": (_abi.F32, torch.float32), "fp64": (_abi.F64, torch.float64)}
CASES = ["below_tile", "tile_minus_1", "tile", "tile_plus_1", "two_tiles_plus_1", "one_column", "empty_columns", "no_nonzeros",
         "rows_empty_later", "dense_row_and_column", "three_panels"]


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def panels_of(case, R):
    """The panels of a case as dense float64 arrays (m x pc), values of order 1."""
    m = {"below_tile": max(R // 2 - 1, 1), "tile_minus_1": R - 1, "tile": R, "tile_plus_1": R + 1}.get(case, 2 * R + 1)
    widths = {"one_column": [1], "rows_empty_later": [70, 70], "three_panels": [70, 1, 67]}.get(case, [70])
    n = sum(widths)
    A = simulate_nmf_sparse(m, max(n, 8), 4, 0.2, seed=len(case) + m)[0].to_scipy().toarray()[:, :n] * (m * max(n, 8) / 4.0)
    if case == "empty_columns":
        A[:, [0, 5, 6, 69]] = 0.0
    if case == "no_nonzeros":
        A[:] = 0.0
    if case == "rows_empty_later":
        A[::3, 70:] = 0.0                      # rows the second panel leaves alone: the first panel's sums must survive
    if case == "dense_row_and_column":
        A[m // 2, :] = 1.0 + A[m // 2, :]
        A[:, 3] = 1.0 + A[:, 3]
    return np.split(A, np.cumsum(widths)[:-1], axis=1)


def dev_csc(A, tdtype):
    c = CSC.from_scipy(sp.csc_matrix(A))
    dev = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", t)
    return dev(c.p), dev(np.append(c.i, 0).astype(np.int32)), dev(np.append(c.x, 0.0), tdtype)


def stream_sums(ctx, dt, tdtype, panels, Hs, k, groups=0):
    m = panels[0].shape[0]
    BW = torch.full((m, k), 7.0, dtype=tdtype, device="cuda")           # overwritten by the first panel
    G = torch.full((k, k), 7.0, dtype=tdtype, device="cuda")
    for q, (A, H) in enumerate(zip(panels, Hs)):
        p, i, x = dev_csc(A, tdtype)
        ctx.stream_rhs_w(dt, p, i, x, A.shape[1], m, H, k, q > 0, BW, groups=groups)
        ctx.stream_gram_accum(dt, H, k, A.shape[1], q > 0, G)
    ctx.sync()
    return BW.cpu().numpy(), G.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("k", [1, 3, 16, 17, 33, 64])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_sums_against_float64(prec, k, case):
    dt, tdtype = DTYPES[prec]
    R = _abi.stream_geometry(dt, k)["tile_rows"]
    panels = panels_of(case, R)
    ctx = _abi.Context(0)
    g = np.random.default_rng(k)
    Hn = [g.uniform(size=(A.shape[1], k)) for A in panels]
    Hs = [torch.from_numpy(h).to("cuda", tdtype) for h in Hn]
    H64 = np.concatenate([h.cpu().numpy().astype(np.float64) for h in Hs])
    A = np.concatenate(panels, axis=1)
    ref_B, ref_G = A.astype(np.float32 if prec == "fp32" else np.float64).astype(np.float64) @ H64, H64.T @ H64
    # the resident ops on the same input: rhs over the CSC of A^T, gram over all of H
    tp, ti, tx = dev_csc(A.T, tdtype)
    Hall = torch.cat(Hs)
    B0 = torch.empty((A.shape[0], k), dtype=tdtype, device="cuda")
    G0 = torch.empty((k, k), dtype=tdtype, device="cuda")
    ctx.rhs(dt, tp, ti, tx, A.shape[0], Hall, k, B0)
    ctx.gram(dt, Hall, k, Hall.shape[0], 0.0, 0.0, G0)
    ctx.sync()
    BW, G = stream_sums(ctx, dt, tdtype, panels, Hs, k)
    dB, dG = rel(B0.cpu().numpy(), ref_B), rel(G0.cpu().numpy(), ref_G.T)
    eB, eG = rel(BW, ref_B), rel(G, ref_G.T)
    print("%s k=%d %s: rhs resident %.3g streamed %.3g | gram resident %.3g streamed %.3g" % (prec, k, case, dB, eB, dG, eG))
    assert eB <= 100 * max(dB, 2.0 ** -52)
    assert eG <= 100 * max(dG, 2.0 ** -52)
    # the same call again, and on two workgroups instead of one per row tile: the same bits
    for groups in (0, 2):
        BW2, G2 = stream_sums(ctx, dt, tdtype, panels, Hs, k, groups=groups)
        assert np.array_equal(BW, BW2) and np.array_equal(G, G2)


def test_gram_finish_matches_gram_of_scaled_factor():
    ctx = _abi.Context(0)
    k, n = 17, 300
    g = np.random.default_rng(3)
    H = torch.from_numpy(g.uniform(size=(n, k))).to("cuda")
    d = torch.from_numpy(g.uniform(0.5, 2.0, size=k)).to("cuda")
    Gacc, G = torch.empty((k, k), dtype=torch.float64, device="cuda"), torch.empty((k, k), dtype=torch.float64, device="cuda")
    ctx.stream_gram_accum(_abi.F64, H, k, n, False, Gacc)
    ctx.stream_gram_finish(_abi.F64, Gacc, d, k, 1e-15, 0.25, G)
    ctx.sync()
    Hs = (H / d).cpu().numpy()
    ref = Hs.T @ Hs + (1e-15 + 0.25) * np.eye(k)
    assert rel(G.cpu().numpy(), ref) <= 100 * 2.0 ** -52 * n


# ---------------------------------------------------------------------------------------------------- the fit against nmf()
@functools.lru_cache(maxsize=None)
def fit_input(name):
    if name == "hawaiibirds":
        d = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
        A = CSC(d["shape"], d["p"], d["i"], d["x"])
    else:
        A = simulate_nmf_sparse(70, 300, 5, 0.3, seed=11)[0]
        A = CSC(A.shape, A.p, A.i, A.x * (70 * 300 / 5.0))
    W0, H0 = O.init_factors(42, 6, A.rows, A.cols, np.float64)
    return A, W0, H0


CONFIGS = {"plain": dict(), "penalised": dict(L1=(0.01, 0.02), L2=(0.03, 0.01), nonneg=(True, False))}


@functools.lru_cache(maxsize=None)
def resident_fit(name, solver, prec, config):
    """nmf() on the input, and its deviation from the float64 oracle fit on w, d, h and the loss"""
    A, W0, H0 = fit_input(name)
    kw = CONFIGS[config]
    mod = nmf(A, 6, tol=0.0, maxit=10, seed=W0, h_init=H0.T.copy(), solver=solver, precision=prec, **kw)
    ref = O.nmf_fit(O.Csc(A.shape, A.p, A.i, A.x), W0, H0, np.float64, max_iter=10, tol=0.0, solver_mode=0 if solver == "cd" else 1,
                    L1=kw.get("L1", (0.0, 0.0)), L2=kw.get("L2", (0.0, 0.0)), nonneg=kw.get("nonneg", (True, True)))
    delta = dict(w=rel(mod.w, ref.W_T), d=rel(mod.d, ref.d), h=rel(mod.h, ref.H.T), loss=rel([mod.misc["loss"]], np.array([ref.loss])))
    return mod, delta


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("solver", ["cd", "cholesky"])
@pytest.mark.parametrize("panel_cols", [64, 300, 1000])
@pytest.mark.parametrize("name", ["hawaiibirds", "random_70x300"])
def test_fit_against_nmf(name, panel_cols, solver, prec, config):
    A, W0, H0 = fit_input(name)
    mod, delta = resident_fit(name, solver, prec, config)
    st = nmf_streaming(A, 6, panel_cols=panel_cols, tol=0.0, maxit=10, seed=W0, h_init=H0.T, solver=solver, precision=prec,
                       **CONFIGS[config])
    got = dict(w=rel(st.w, mod.w), d=rel(st.d, mod.d), h=rel(st.h, mod.h), loss=rel([st.misc["loss"]], np.array([mod.misc["loss"]])))
    print(name, panel_cols, solver, prec, config, "nmf vs float64:", delta, "streamed vs nmf:", got)
    pc = min(panel_cols, A.cols)
    assert st.misc["panel_cols"] == pc and st.misc["panels"] == -(-A.cols // pc) and st.misc["iter"] == 10
    widest = max(int(A.p[min(j + pc, A.cols)] - A.p[j]) for j in range(0, A.cols, pc))
    assert st.misc["panel_bytes_peak"] <= 2 * (4 * (pc + 1) + 12 * widest)
    for key in got:
        assert got[key] <= 100 * max(delta[key], 2.0 ** -52), (key, got[key], delta[key])


# ---------------------------------------------------------------------------------------------------- .spz input
SPZ = os.path.join(ROOT, "tests", "golden", "pbmc3k.spz")


@functools.lru_cache(maxsize=None)
def pbmc3k():
    """(the matrix read through the whole-file device decoder, the file's chunk width)"""
    raw = np.fromfile(SPZ, np.uint8)
    st, m, n, nnz, _ = _abi.spz_info(raw)
    assert st == 0
    ctx = _abi.Context(0)
    p, i = (torch.empty(c, dtype=torch.int32, device="cuda") for c in (n + 1, nnz))
    x = torch.empty(nnz, dtype=torch.float64, device="cuda")
    ctx.spz_decode(raw, p, i, x)
    ctx.sync()
    return CSC((m, n), p.cpu().numpy(), i.cpu().numpy(), x.cpu().numpy()), int(raw[24:28].view(np.uint32)[0])


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("width", ["one_chunk", "all_chunks"])
def test_spz_path_equals_csc_of_the_same_matrix(width, prec):
    A, chunk = pbmc3k()
    pc = chunk if width == "one_chunk" else A.cols
    kw = dict(panel_cols=pc, tol=0.0, maxit=3, seed=5, precision=prec)
    a, b = nmf_streaming(SPZ, 8, **kw), nmf_streaming(A, 8, **kw)
    assert a.misc["panels"] == b.misc["panels"] == -(-A.cols // pc) and a.misc["panel_cols"] == b.misc["panel_cols"]
    # the panel boundaries coincide (whole chunks), so the two fits run the same operations on the same numbers
    assert np.array_equal(a.w, b.w) and np.array_equal(a.d, b.d) and np.array_equal(a.h, b.h) and a.misc["loss"] == b.misc["loss"]
    assert a.misc["panel_bytes_peak"] == b.misc["panel_bytes_peak"]
    resident = 2 * 12 * A.nnz + 4 * (A.rows + A.cols + 2)
    print(width, prec, "panel bytes", a.misc["panel_bytes_peak"], "range table", a.misc["range_table_bytes"], "resident CSC + transpose", resident)
    if width == "one_chunk":
        assert a.misc["panel_bytes_peak"] + a.misc["range_table_bytes"] < resident / 4


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(mask="zeros"), dict(loss="nb"), dict(robust=True), dict(test_fraction=0.1), dict(L21=(0.1, 0.0)),
                                dict(angular=(0.0, 0.1)), dict(graph_W=np.eye(70)), dict(target_H=np.ones((6, 300))),
                                dict(projective=True), dict(symmetric=True), dict(seed="lanczos"), dict(devices=2), dict(zi="row")])
def test_python_refusals_name_the_option(kw):
    A = fit_input("random_70x300")[0]
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        nmf_streaming(A, 6, **kw)


@pytest.mark.parametrize("change, word", [(dict(k=65), "k > 64"), (dict(devices=2), "devices"), (dict(spz="no_such_file.spz"), ".spz")])
def test_entry_refusals_leave_outputs_untouched(change, word):
    A, W0, H0 = fit_input("random_70x300")
    k = change.get("k", 6)
    W, H = np.full((A.rows, k), 0.5), np.full((A.cols, k), 0.25)
    r = _abi.nmf_streaming(None if "spz" in change else (A.p, A.i, A.x), change.get("spz"), A.rows, A.cols, k, W, H,
                           devices=change.get("devices", 1))
    assert r["status"] == -1 and word in r["error"]
    assert np.all(W == 0.5) and np.all(H == 0.25)
