"""GPU constrained block SVD, KSPR (rcppml_gpu_svd_krylov_ex, rcppml_gpu_svd_krylov_dense_ex: rcppml_amd/csrc/ops_svd.hip,
kernels_svd_krylov.hip.h) against the numpy restatement of the reference's CPU path (tests/svd_krylov_ref.py), against the Lanczos
entries bit for bit where the seed must coincide, and through the Python surface.

Tolerances are per case: the device is held to four times the restatement's own deviation on that case -- its float32 run against
its float64 run for fp32, its float64 run against its np.longdouble run for fp64 (svd_krylov_ref.MEASURED, by
svd_krylov_ref.deviation: u, d, v and dW together)."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_krylov_ref as K
from rcppml_amd import _abi, svd as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def parts(A):
    M = sp.csc_matrix(A)
    M.sort_indices()
    return (M.indptr, M.indices, M.data, A.shape[0], A.shape[1])


def abi_kw(kw):
    kw = dict(kw)
    if "ub" in kw:
        kw["upper_bound"] = kw.pop("ub")
    return kw


def run_gpu(A, k, dense=False, **kw):
    r = _abi.svd_krylov(A if dense else parts(A), k, dense=dense, **abi_kw(kw))
    assert r["status"] == 0, r["error"]
    return r


def as_result(r):
    k = r["k"]
    return dict(u=r["U"][:, :k], s=r["d"][:k], v=r["V"][:, :k], dw=r["dw"])


@functools.lru_cache(maxsize=None)
def reference(m, n, k, name):
    return K.kspr(K.case_input(m, n)[0], K.seed_of(m, n, k), K.PASSES, 0.0, **K.CONSTRAINTS[name])


def check_case(m, n, k, name, precision, dense=False):
    A, V0 = K.case_input(m, n)[0], K.seed_of(m, n, k)
    assert not A[3].any() and not A[:, 5].any()                 # the empty row and column
    ref = reference(m, n, k, name)
    if name == "nonneg" and k > 1:
        assert np.sum(ref["d"] == 0) >= 1                       # the dead-column rule is exercised
    r = run_gpu(A, k, dense=dense, precision=precision, tol=0.0, max_iter=K.PASSES, V0=V0, **K.CONSTRAINTS[name])
    assert (r["passes"], r["k"]) == (ref["passes"], k) and r["dw"].size == K.PASSES - 1
    dev = K.deviation(as_result(r), ref, align=name == "l2")
    bound = 4 * K.MEASURED[(m, n, k, name)][0 if precision == "float" else 1]
    print("%s %s dense=%s: deviation %.3e bound %.3e" % ((m, n, k, name), precision, dense, dev, bound))
    assert dev <= bound
    if K.CONSTRAINTS[name].get("center"):
        assert np.allclose(r["row_means"], A.mean(axis=1), rtol=1e-12, atol=0)
    assert abs(r["frob"] - (np.sum(A * A) - (A.shape[1] * np.sum(A.mean(axis=1) ** 2) if K.CONSTRAINTS[name].get("center") else 0))) \
        <= 1e-12 * np.sum(A * A)


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("name", list(K.CONSTRAINTS))
@pytest.mark.parametrize("m, n, k", K.SHAPES)
def test_seeded_parity(m, n, k, name, precision):
    check_case(m, n, k, name, precision)


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("name", list(K.CONSTRAINTS))
def test_seeded_parity_dense(name, precision):
    check_case(130, 67, 17, name, precision, dense=True)


def test_nonneg_output_is_nonnegative_and_ordered():
    m, n, k = 130, 67, 16
    r = run_gpu(K.case_input(m, n)[0], k, precision="float", tol=0.0, max_iter=K.PASSES, V0=K.seed_of(m, n, k), nonneg=(True, True))
    assert np.all(r["U"] >= 0) and np.all(r["V"] >= 0) and np.all(np.diff(r["d"][:k]) <= 0)
    assert r["d"][k - 1] == 0 and not r["U"][:, k - 1].any() and not r["V"][:, k - 1].any()      # the dead factor sorts last


# ------------------------------------------------------------------------------------------------ convergence
def test_convergence_stops_at_the_restatements_pass():
    """tol sits between two passes of the restatement with a factor two to spare on either side, so the stopping pass does not
    hang on rounding."""
    A, V0, k, tol, kw = K.convergence_input()
    ref = K.kspr(A, V0, 0, tol, **kw)
    print("restatement dW", ref["dw"], "passes", ref["passes"])
    assert 2 < ref["passes"] < K.pass_limit(k)
    assert ref["dw"][-1] < tol / 2 and ref["dw"][-2] > 2 * tol
    for precision in ("double", "float"):
        r = run_gpu(A, k, precision=precision, tol=tol, max_iter=0, V0=V0, **kw)
        print(precision, "device dW", r["dw"])
        assert r["passes"] == ref["passes"] and r["dw"].size == ref["passes"] - 1
        assert np.allclose(r["dw"], ref["dw"], rtol=1e-3 if precision == "float" else 1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ the full path
@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True])
def test_null_seed_is_the_lanczos_seed_bit_for_bit(precision, dense):
    m, n, k = 130, 67, 16
    A = K.case_input(m, n)[0]
    kw = dict(precision=precision, center=True, seed=3, tol=1e-5)
    lz = _abi.svd_pca(A if dense else parts(A), k, dense=dense, algorithm=2, max_iter=0, **kw)
    assert lz["status"] == 0 and lz["k"] == k
    a = run_gpu(A, k, dense=dense, max_iter=4, nonneg=(True, True), **kw)
    b = run_gpu(A, k, dense=dense, max_iter=4, nonneg=(True, True), V0=lz["V"][:, :k], **kw)
    assert a["passes"] == b["passes"] and a["k"] == b["k"] == k
    for key in ("U", "d", "V", "dw", "row_means"):
        assert np.array_equal(a[key], b[key]), key
    assert a["frob"] == b["frob"]


def test_rank_deficient_input_selects_what_lanczos_selects():
    rng = np.random.default_rng(5)
    A = np.abs(rng.standard_normal((60, 5))) @ np.abs(rng.standard_normal((5, 40)))
    for precision in ("double", "float"):
        lz = _abi.svd_pca(parts(A), 8, algorithm=2, max_iter=0, precision=precision, seed=1, tol=1e-5)
        assert lz["status"] == 0
        r = run_gpu(A, 8, precision=precision, seed=1, tol=1e-5, max_iter=3, nonneg=(True, True))
        assert r["k"] == lz["k"]
        assert not r["U"][:, r["k"]:].any() and not r["d"][r["k"]:].any()        # nothing written past k_actual


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("m, n, k", [(130, 67, 17), (200, 150, 128)])
def test_two_runs_are_bitwise_identical(m, n, k, precision):
    A = K.case_input(m, n)[0]
    kw = dict(precision=precision, center=True, max_iter=4, tol=0.0, nonneg=(True, False), L1=(0.0, 0.01), L2=(0.05, 0.0))
    a, b = run_gpu(A, k, **kw), run_gpu(A, k, **kw)
    for key in ("U", "d", "V", "dw"):
        assert np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ surface
def test_python_surface():
    z = np.load(os.path.join(HERE, "golden", "hawaiibirds.npz"))
    A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    A.sort_indices()
    r = S.svd(A, k=10, nonneg=True, method="krylov")
    mi = r["misc"]
    assert np.all(r["u"] >= 0) and np.all(r["v"] >= 0) and np.all(np.diff(r["d"]) <= 0)
    assert mi["method"] == "krylov" and mi["passes"] >= 2 and len(mi["dw"]) == mi["passes"] - 1
    assert len(mi["iters_per_factor"]) == 0 and r["u"].shape == (183, 10) and r["v"].shape == (1183, 10)
    with pytest.raises(_abi.BackendError) as e:
        S.svd(A, k=10, nonneg=True)
    assert 'method = "krylov"' in str(e.value) and 'method = "deflation"' in str(e.value)
    assert S.svd(A, k=4, method="krylov", precision="double")["misc"]["method"] == "krylov"      # unconstrained: Lanczos
