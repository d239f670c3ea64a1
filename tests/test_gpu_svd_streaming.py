"""GPU checks of the panel-streamed randomized SVD (csrc/ops_stream_svd.hip): the scatter block product against
numpy float64 under the standard bound of a sum of products, its independence of the grid, svd_streaming() against
svd(method = "randomized") under the rule of DESIGN.md section 7 (delta = the resident call's deviation from tests/svd_rand_ref.py in
float64; the streamed call gets 100 * max(delta, eps)), .spz against CSC, repeatability and the refusals."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import svd_rand_ref as RR
from rcppml_amd import _abi, pca_streaming, svd_streaming
from rcppml_amd.data import CSC
from rcppml_amd.svd import svd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPZ = os.path.join(ROOT, "tests", "golden", "pbmc3k.spz")
DTYPES = {"fp32": (_abi.F32, torch.float32, np.float32, 2.0 ** -24), "fp64": (_abi.F64, torch.float64, np.float64, 2.0 ** -53)}
PREC = {"fp32": "float", "fp64": "double"}


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def panels_of(m):
    """Three panels (m x 64, m x 100, m x 1) as dense float64: an empty column, an empty row, one dense column, and the last panel
    empty.  About a third of the entries are set, so an 8-row slice of a column holds 0 to 8 of them."""
    g = np.random.default_rng(m)
    A = g.uniform(0.5, 1.5, size=(m, 165)) * (g.uniform(size=(m, 165)) < 0.3)
    A[:, 7] = 0.0
    A[:, 20] = g.uniform(0.5, 1.5, size=m)
    A[m // 3, :] = 0.0
    A[:, 164] = 0.0
    return np.split(A, [64, 164], axis=1)


def block_prod(prec, l, m, groups=0):
    """(Y from the device as l x m accumulated over the panels, the float64 reference, |A| |X|, nonzeros per row)"""
    dt, tdtype, ndtype, _ = DTYPES[prec]
    ctx = _abi.Context(0)
    g = np.random.default_rng(l)
    Y = torch.full((m, l), 7.0, dtype=tdtype, device="cuda")               # overwritten by the first panel
    ref, mag, cnt = np.zeros((m, l)), np.zeros((m, l)), np.zeros(m)
    dev = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", t)
    for q, A in enumerate(panels_of(m)):
        c = CSC.from_scipy(sp.csc_matrix(A))
        X = dev(g.uniform(-1, 1, size=(A.shape[1], l)), tdtype)
        x = dev(np.append(c.x, 0.0), tdtype)
        _abi.stream_block_prod(ctx, dt, dev(c.p), dev(np.append(c.i, 0).astype(np.int32)), x, m, A.shape[1], l, X, q > 0, Y, groups=groups)
        A64, X64 = A.astype(ndtype).astype(np.float64), X.cpu().numpy().astype(np.float64)
        ref, mag, cnt = ref + A64 @ X64, mag + np.abs(A64) @ np.abs(X64), cnt + (A != 0).sum(axis=1)
    ctx.sync()
    return Y.cpu().numpy().astype(np.float64), ref, mag, cnt


@pytest.mark.parametrize("tall", [False, True])
@pytest.mark.parametrize("l", [1, 5, 32, 33, 64, 65, 128])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_block_product_against_float64(prec, l, tall):
    m = _abi.stream_block_geometry(DTYPES[prec][0], l)["tile_rows"] + 1 if tall else 70
    Y, ref, mag, cnt = block_prod(prec, l, m)
    u = DTYPES[prec][3]
    gamma = (cnt + 1) * u / (1 - (cnt + 1) * u)
    excess = np.abs(Y - ref) - gamma[:, None] * mag
    print("%s l=%d m=%d: max |got - ref| %.3g, largest (error - bound) %.3g" % (prec, l, m, np.abs(Y - ref).max(), excess.max()))
    assert np.all(excess <= 0)
    for groups in (1, 7):                       # the same bits from one workgroup and from seven
        assert np.array_equal(Y, block_prod(prec, l, m, groups=groups)[0])


# ---------------------------------------------------------------------------------------------------- the fit against svd()
@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "hawaiibirds":
        z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
        A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    else:                                       # 200 x 400, a third of the entries set, columns scaled down geometrically
        g = np.random.default_rng(4)
        A = sp.csc_matrix(g.uniform(0.5, 1.5, size=(200, 400)) * (g.uniform(size=(200, 400)) < 0.3) * 0.97 ** np.arange(400))
    A.sort_indices()
    return A


def d_and_product(r):
    return r["d"], (r["u"] * r["d"]) @ r["v"].T


@functools.lru_cache(maxsize=None)
def resident(name, k, center, prec):
    """svd(method = "randomized") on the input, and its deviation from the float64 restatement on d and on u d v'"""
    r = svd(matrix(name), k, method="randomized", center=center, seed=7, precision=PREC[prec])
    ref = RR.randomized_svd(matrix(name).toarray(), k, maxit=3, center=center, seed=7)
    d, P = d_and_product(r)
    return d, P, rel(d, ref["d"]), rel(P, (ref["u"] * ref["d"]) @ ref["v"].T)


def check_against_resident(name, k, center, prec, panel_cols):
    A = matrix(name)
    d0, P0, dd, dP = resident(name, k, center, prec)
    st = svd_streaming(A, k, center=center, seed=7, precision=PREC[prec], panel_cols=panel_cols)
    d, P = d_and_product(st)
    ed, eP, eps = rel(d, d0), rel(P, P0), 2.0 ** -23 if prec == "fp32" else 2.0 ** -52
    print("%s k=%d center=%d %s panel_cols=%d: svd() vs float64 d %.3g product %.3g | streamed vs svd() d %.3g product %.3g"
          % (name, k, center, prec, panel_cols, dd, dP, ed, eP))
    pc = min(panel_cols, A.shape[1])
    assert st["misc"]["panels"] == -(-A.shape[1] // pc) and st["misc"]["passes"] == 2 * 3 + 2 + int(center)
    assert ed <= 100 * max(dd, eps) and eP <= 100 * max(dP, eps)
    if center:      # a row of nnz_r non-negative values rounded to the dtype, summed in any order, divided once: gamma_(nnz_r + 2)
        terms = np.bincount(A.indices, minlength=A.shape[0]).max() + 2
        assert A.data.min() >= 0
        assert rel(st["misc"]["row_means"], np.asarray(A.mean(axis=1)).ravel()) <= terms * eps / 2 / (1 - terms * eps / 2)


@pytest.mark.parametrize("panel_cols", [256, 1183])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("k", [4, 40])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_against_svd_randomized(prec, k, center, panel_cols):
    check_against_resident("hawaiibirds", k, center, prec, panel_cols)


def test_widest_sketch():
    assert RR.sizes(200, 400, 107)[1] == 128
    check_against_resident("decaying_200x400", 107, False, "fp64", 150)      # panels that split a record block of 16 columns


def test_spz_equals_csc_and_two_runs_are_identical():
    raw = np.fromfile(SPZ, np.uint8)
    st, m, n, nnz, _ = _abi.spz_info(raw)
    assert st == 0
    ctx = _abi.Context(0)
    p, i = (torch.empty(c, dtype=torch.int32, device="cuda") for c in (n + 1, nnz))
    x = torch.empty(nnz, dtype=torch.float64, device="cuda")
    ctx.spz_decode(raw, p, i, x)
    ctx.sync()
    A = CSC((m, n), p.cpu().numpy(), i.cpu().numpy(), x.cpu().numpy())
    kw = dict(maxit=1, seed=3, panel_cols=1024)
    a, b, c = svd_streaming(SPZ, 10, **kw), svd_streaming(A, 10, **kw), svd_streaming(A, 10, **kw)
    assert a["misc"]["panels"] == b["misc"]["panels"] == 3 and a["misc"]["passes"] == 4
    assert np.array_equal(a["d"], b["d"])
    assert all(np.array_equal(b[key], c[key]) for key in ("u", "d", "v"))


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(L1=0.1), dict(L2=(0.0, 0.1)), dict(nonneg=True), dict(upper_bound=1.0), dict(method="lanczos"),
                                dict(method="krylov"), dict(k="auto"), dict(test_fraction=0.1), dict(mask="zeros"), dict(L21=0.1),
                                dict(angular=0.1), dict(graph_U=np.eye(183)), dict(graph_lambda=0.5), dict(devices=2)])
def test_python_refusals_name_the_option(kw):
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        pca_streaming(matrix("hawaiibirds"), **kw)


@pytest.mark.parametrize("change, word", [(dict(k=108), "k:"), (dict(devices=2), "devices"), (dict(spz="no_such_file.spz"), ".spz")])
def test_entry_refusals_leave_outputs_untouched(change, word):
    A = matrix("decaying_200x400")
    k = change.get("k", 6)
    b = {key: np.full(size, -7.0) for key, size in (("U", 200 * k), ("d", k), ("V", 400 * k), ("row_means", 200))}
    r = _abi.svd_streaming(None if "spz" in change else (A.indptr, A.indices, A.data), change.get("spz"), 200, 400, k, center=True,
                           devices=change.get("devices", 1), buffers=b)
    assert r["status"] == -1 and word in r["error"]
    assert all(np.all(v == -7.0) for v in b.values())
