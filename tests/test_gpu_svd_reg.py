"""GPU L21 / angular / graph-regularised deflation SVD (rcppml_gpu_svd_reg_ex, rcppml_gpu_svd_reg_dense_ex: rcppml_amd/csrc/ops_svd.hip,
kernels_svd_reg.hip.h) against the numpy restatement of the reference's CPU loop (tests/svd_reg_ref.py), against the cv entries bit
for bit with every term off, and through the Python surface.

Bounds.  fp64: u, d, v (each relative to its largest reference magnitude) and every test loss within 1e-10 of the float64
restatement, with equal iters, k, k_computed and n_test -- the yardstick test_gpu_svd_cv.assert_parity applies to the same loop; the
restatement's own float64-vs-longdouble deviation is below 1e-11 on every case (tests/test_svd_reg_cpu.py), so a decade of the bound
is the device's alone.  fp32: four times svd_reg_ref.MEASURED[case], the restatement's own float32-vs-float64 deviation on that case,
with the same counts; four is the factor test_gpu_svd_cv and test_gpu_svd_krylov use for the same comparison.  The fixed iteration
counts hold because no iteration of a case comes within 100 eps of convergence (tests/test_svd_reg_cpu.py)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_cv_ref as C
import svd_reg_ref as R
from rcppml_amd import _abi, svd as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def parts_of(A, keep):
    cols, rows = np.nonzero(keep.T)
    p = np.concatenate([[0], np.cumsum(keep.sum(axis=0))]).astype(np.int32)
    return (p, rows.astype(np.int32), A[rows, cols].astype(np.float64), A.shape[0], A.shape[1])


def mask_of(mask):
    cols, rows = np.nonzero(mask.T)
    p = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int32)
    return (p, rows.astype(np.int32), mask.shape[0], mask.shape[1])


def gpu_kwargs(kw):
    """The keywords of reg_deflation_svd as _abi.svd_reg takes them."""
    kw = dict(kw)
    out = dict(max_iter=kw.pop("maxit"))
    lam = kw.pop("graph_lambda", (0, 0))
    for side, l in (("graph_u", lam[0]), ("graph_v", lam[1])):
        g = kw.pop(side, None)
        if g is not None:
            out[side] = R.graph_csc(g, l)
    if kw.get("obs_mask") is not None:
        kw["obs_mask"] = mask_of(kw["obs_mask"])
    out.update(kw)
    return out


def run_gpu(A, keep, kw, precision, call=None, k=R.K):
    src = A if keep is None else parts_of(A, keep)
    r = (call or _abi.svd_reg)(src, k, dense=keep is None, precision=precision, **gpu_kwargs(kw))
    assert r["status"] == 0, r["error"]
    return r


def as_result(r):
    ks = r["k"]
    return dict(u=r["U"][:, :ks], d=r["d"][:ks], v=r["V"][:, :ks])


def assert_counts(r, ref):
    kc = ref["k_computed"]
    assert (r["k"], r["k_computed"], r["n_test"], r["n_masked"]) == (ref["k_selected"], kc, ref["n_test"], ref["n_masked"])
    assert np.array_equal(r["iters"][:kc], ref["iters"])


# ------------------------------------------------------------------------------------------------ parity at fixed iterations
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%s" % c)
def test_fp64_parity(case):
    A, keep, kw = R.case_kwargs(*case)
    ref = R.case_ref(*case)
    r = run_gpu(A, keep, kw, "double")
    assert_counts(r, ref)
    dev = R.deviation(as_result(r), ref)
    print("%s-%s double: deviation %.3e bound 1e-10" % (case + (dev,)))
    assert dev <= 1e-10
    tl, kc = ref["test_loss"], ref["k_computed"]
    if tl.size:
        assert np.all(np.abs(r["test_loss"][:kc] - tl) <= 1e-10 * tl)
    if kw.get("center"):
        assert np.allclose(r["row_means"], ref["row_means"], rtol=1e-12, atol=0)
    assert abs(r["frob"] - ref["frob"]) <= 1e-12 * abs(ref["frob"])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%s" % c)
def test_fp32_parity(case):
    A, keep, kw = R.case_kwargs(*case)
    ref = R.case_ref(*case)
    r = run_gpu(A, keep, kw, "float")
    assert_counts(r, ref)
    dev, bound = R.deviation(as_result(r), ref), 4 * R.MEASURED[case]
    print("%s-%s float: deviation %.3e bound %.3e share %.2f" % (case + (dev, bound, dev / bound)))
    assert dev <= bound


# ------------------------------------------------------------------------------------------------ convergence
@pytest.mark.parametrize("dt, precision", [(np.float32, "float"), (np.float64, "double")])
def test_converged_factors_stop_at_the_restatements_iteration(dt, precision):
    A, keep, kw = R.convergence_kwargs(dt)
    ref = R.reg_deflation_svd(A, R.K, stored=keep, dtype=dt, **kw)
    r = run_gpu(A, keep, kw, precision)
    print("iters", r["iters"][:R.K], ref["iters"])
    assert_counts(r, ref)


# ------------------------------------------------------------------------------------------------ identity and repeatability
@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("cv", [False, True])
def test_with_every_term_off_the_entry_is_the_cv_entry_bit_for_bit(name, precision, cv):
    A, keep = (C.dense_input(), None) if name == "dense" else C.sparse_input()
    kw = dict(maxit=200, tol=1e-5, center=True, nonneg=(False, True))
    if cv:
        kw.update(test_fraction=0.1, patience=3)
    k = C.K_MAX if cv else 4
    a = run_gpu(A, keep, kw, precision, k=k)
    b = run_gpu(A, keep, kw, precision, call=_abi.svd_cv, k=k)
    for key in ("U", "d", "V", "iters", "test_loss", "row_means"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["k"], a["k_computed"], a["n_test"], a["frob"]) == (b["k"], b["k_computed"], b["n_test"], b["frob"])
    # zero-valued terms and a graph with lambda 0 are off as well
    g = R.graph_csc(R.ring_laplacian(A.shape[1], 1), 0.0)
    src = A if keep is None else parts_of(A, keep)
    c = _abi.svd_reg(src, k, dense=keep is None, precision=precision, L21=(0, 0), angular=(0, 0), graph_v=g, **gpu_kwargs(kw))
    assert c["status"] == 0 and np.array_equal(c["U"], b["U"]) and np.array_equal(c["V"], b["V"])


@pytest.mark.parametrize("precision", ["float", "double"])
def test_two_runs_with_every_term_on_are_bitwise_identical(precision):
    case = ("sparse2100x70", "all_l1_cv")
    A, keep, kw = R.case_kwargs(*case)
    a, b = run_gpu(A, keep, kw, precision), run_gpu(A, keep, kw, precision)
    for key in ("U", "d", "V", "iters", "test_loss"):
        assert np.array_equal(a[key], b[key]), key
    off = {key: v for key, v in kw.items() if key not in ("L21", "angular", "graph_u", "graph_v", "graph_lambda")}
    plain = run_gpu(A, keep, off, precision, call=_abi.svd_cv)
    assert R.deviation(as_result(a), dict(u=plain["U"][:, :a["k"]], d=plain["d"][:a["k"]], v=plain["V"][:, :a["k"]])) > 1e-3


# ------------------------------------------------------------------------------------------------ surface
def birds():
    z = np.load(os.path.join(HERE, "golden", "hawaiibirds.npz"))
    A = sp.csc_matrix((z["x"], z["i"], z["p"]), shape=tuple(z["shape"]))
    L = sp.csc_matrix(R.graph_dense(R.ring_laplacian(A.shape[1], 4)))
    return A, L


def test_surface_on_hawaiibirds():
    A, L = birds()
    kw = dict(L21=0.1, angular=0.2, graph_V=L, graph_lambda=(0, 0.02))
    r = S.svd(A, k=4, **kw)
    plain = S.svd(A, k=4, method="deflation")
    assert r["misc"]["method"] == "deflation" and r["u"].shape == (A.shape[0], 4) and r["v"].shape == (A.shape[1], 4) and r["d"].shape == (4,)
    assert np.all(np.isfinite(r["u"])) and np.all(np.isfinite(r["v"])) and np.all(r["d"] > 0)
    assert R.deviation(r, plain) > 1e-4                       # far above fp32 rounding
    # k = "auto" is k = k_max: below 8 so that method "auto" stays with deflation, as R resolves it (at the default k_max = 50 it is
    # krylov, which is refused like k = 10 below)
    auto = S.svd(A, k="auto", k_max=7, **kw)
    m = auto["misc"]
    assert m["auto_rank"] and m["method"] == "deflation" and m["n_test"] > 0
    assert 1 <= m["k_selected"] <= len(m["test_loss"]) <= 7 and len(auto["d"]) == m["k_selected"] and np.all(m["test_loss"] > 0)
    for k in (10, "auto"):
        with pytest.raises(_abi.BackendError):
            S.svd(A, k=k, **kw)


def test_the_reference_entries_still_refuse_l21():
    A = C.dense_input()
    r = _abi.svd_pca(A, 3, dense=True, L21=(0.1, 0.0))
    assert r["status"] == -1 and "L21" in r["error"]
