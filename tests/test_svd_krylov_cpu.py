"""CPU checks of the constrained krylov SVD (KSPR): the numpy restatement (tests/svd_krylov_ref.py, the GPU path's parity target)
against brute force, the ABI declarations and the refusals that hold before any device work, and the routes of svd().  No GPU
needed."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import svd_krylov_ref as K
from rcppml_amd import _abi, svd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_a_pass_from_an_exact_singular_subspace_returns_it():
    A = K.case_input(70, 45)[0]
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    r = K.kspr(A, Vt[:6].T, 3, 0.0, L2=(0.0, 0.0))            # no active projection
    assert r["passes"] == 3 and np.all(r["dw"] < 1e-12)
    assert np.allclose(np.abs(np.sum(r["W"] * U[:, :6], axis=0)), 1, atol=1e-12)
    assert np.allclose(np.abs(np.sum(r["V"] * Vt[:6].T, axis=0)), 1, atol=1e-12)
    assert np.allclose(r["s"], s[:6], rtol=1e-10)


@pytest.mark.parametrize("L1, nonneg, ub", [(0.3, False, 0.0), (0.0, True, 0.0), (0.2, True, 0.4), (0.0, False, 0.25)])
def test_project_and_normalize_against_a_loop(L1, nonneg, ub):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((9, 4))
    nsq = np.array([1.0, 0.5, 2.0, 1.5])
    want, dwant = X.copy(), np.zeros(4)
    for c in range(4):
        for i in range(9):
            v, thr = want[i, c], L1 / (2 * nsq[c])
            if L1 > 0:
                v = v - thr if v > thr else (v + thr if v < -thr else 0.0)
            if nonneg:
                v = max(v, 0.0)
            if ub > 0:
                v = min(v, ub)
            want[i, c] = v
        dwant[c] = np.sqrt(sum(want[i, c] ** 2 for i in range(9)))
        want[:, c] /= dwant[c]
    got = X.copy()
    d = K.project_and_normalize(got, L1, nonneg, ub, nsq, 100 * np.finfo(float).eps)
    assert np.allclose(got, want, rtol=1e-14, atol=0) and np.allclose(d, dwant, rtol=1e-14)


def test_dead_column_rule():
    X = np.array([[1.0, -1.0, 1e-15], [2.0, -2.0, 0.0]])
    d = K.project_and_normalize(X, 0.0, True, 0.0, np.array([0.0, 1.0, 1.0]), 100 * np.finfo(float).eps)
    assert np.array_equal(d, [0, 0, 0])
    assert not X[:, 0].any() and not X[:, 1].any()                 # nsq <= 0 zeroes; nonneg leaves nothing
    assert X[0, 2] == 1e-15                                        # a norm below 100 eps gives d = 0 and leaves the column
    r = K.kspr(K.case_input(70, 45)[0], K.seed_of(70, 45, 8), 4, 0.0, nonneg=(True, True))
    dead = np.flatnonzero(r["d"] == 0)
    assert dead.size >= 1 and not r["W"][:, dead].any() and not r["V"][:, dead].any()
    assert np.all(np.isfinite(r["W"])) and np.all(np.isfinite(r["V"]))


def test_pass_limit_formula():
    assert [K.pass_limit(k) for k in (1, 8, 16, 17, 64, 65, 128)] == [10, 10, 11, 13, 15, 17, 17]
    assert K.pass_limit(128, 4) == 4
    assert [_abi.krylov_pass_limit(k) for k in (1, 8, 16, 17, 64, 65, 128)] == [K.pass_limit(k) for k in (1, 8, 16, 17, 64, 65, 128)]


def test_phase3_sort_is_stable_by_d_then_index():
    W, V = np.arange(12.0).reshape(3, 4), np.arange(8.0).reshape(2, 4)
    u, s, v = K.phase3(W, np.array([0.0, 2.0, 0.0, 2.0]), V, True)
    assert np.array_equal(s, [2, 2, 0, 0])
    assert np.array_equal(u, W[:, [1, 3, 0, 2]]) and np.array_equal(v, V[:, [1, 3, 0, 2]])


def test_l2_only_extraction_is_the_svd_of_the_product():
    rng = np.random.default_rng(4)
    W, V, d = rng.standard_normal((20, 5)), rng.standard_normal((12, 5)), rng.random(5) + 0.5
    u, s, v = K.extract(W, d, V)
    U0, s0, Vt0 = np.linalg.svd((W * d) @ V.T)
    assert np.allclose(s, s0[:5], rtol=1e-12)
    sg = np.sign(np.sum(u * U0[:, :5], axis=0))
    assert np.allclose(u * sg, U0[:, :5], atol=1e-10) and np.allclose(v * sg, Vt0[:5].T, atol=1e-10)


def test_measured_deviations_cover_every_case():
    assert set(K.MEASURED) == {(m, n, k, name) for m, n, k in K.SHAPES for name in K.CONSTRAINTS}
    m, n, k, name = 70, 45, 8, "nonneg"                            # one case re-measured: the constants are the restatement's
    A, V0 = K.case_input(m, n)[0], K.seed_of(m, n, k)
    r = {dt: K.kspr(A, V0, K.PASSES, 0.0, dtype=dt, **K.CONSTRAINTS[name]) for dt in (np.float32, np.float64)}
    assert 0.25 < K.deviation(r[np.float32], r[np.float64]) / K.MEASURED[(m, n, k, name)][0] < 4


# ------------------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entries_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_svd_krylov_ex", 31), ("rcppml_gpu_svd_krylov_dense_ex", 28)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert m.group(1).count("*") == count and len(m.group(1).split(",")) == count, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name), name


def _csc(A):
    M = sp.csc_matrix(A)
    M.sort_indices()
    return (M.indptr, M.indices, M.data, A.shape[0], A.shape[1])


@pytest.mark.parametrize("kw, msg", [
    (dict(k=0), "k_max must be in [1, min(m, n)]"),
    (dict(k=21), "k_max must be in [1, min(m, n)]"),
    (dict(tol=-1.0), "tol must be non-negative"),
    (dict(L1=(-0.1, 0)), "L1 penalties must be non-negative"),
    (dict(L2=(0, -0.1)), "L2 penalties must be non-negative"),
    (dict(upper_bound=(-1, 0)), "upper bounds must be non-negative"),
    (dict(nonneg=(False, False)), "the krylov method without element constraints is Lanczos: call rcppml_gpu_svd_pca_* with algorithm 2"),
    (dict(V0="nan"), "V0 holds a non-finite value"),
])
def test_abi_refusals_leave_buffers_untouched(kw, msg):
    """Refused before any device work, so these hold with or without a GPU."""
    A = np.abs(np.random.default_rng(2).standard_normal((30, 20)))
    kw = dict(dict(nonneg=(True, True)), **kw)
    k = kw.pop("k", 3)
    kb = max(k, 1)
    if kw.get("V0") == "nan":
        kw["V0"] = np.full((20, k), np.nan)
    for dense in (False, True):
        for precision in ("double", "float"):
            bufs = dict(U=np.full(30 * kb, 7.0), d=np.full(kb, 7.0), V=np.full(20 * kb, 7.0), row_means=np.full(30, 7.0),
                        dw=np.full(32, 7.0))
            r = _abi.svd_krylov(A if dense else _csc(A), k, dense=dense, precision=precision, center=True, buffers=bufs, **kw)
            assert (r["status"], r["error"]) == (-1, msg)
            assert all(np.all(b == 7) for b in bufs.values())
            assert (r["k"], r["passes"], r["frob"], r["wall_ms"]) == (0, 0, 0.0, 0.0)


def test_abi_refuses_k_above_128_and_a_malformed_csc():
    A = sp.random(140, 135, density=0.2, format="csc", random_state=1)
    r = _abi.svd_krylov(_csc(A.toarray()), 129, nonneg=(True, True))
    assert (r["status"], r["error"]) == (-1, "k_max above 128 is not supported by the krylov method")
    x = np.array([1.0, 2.0, 3.0])
    for p, i, msg in (([1, 2, 3], [0, 2, 1], "col_ptr must start at 0 and end at nnz"), ([0, 4, 3], [0, 2, 1], "col_ptr must be non-decreasing"),
                      ([0, 2, 3], [0, 3, 1], "row index out of range")):
        r = _abi.svd_krylov((p, i, x, 3, 2), 1, nonneg=(True, True))
        assert (r["status"], r["error"]) == (-1, msg)


def test_reference_entries_keep_refusing_constrained_krylov():
    A = np.abs(np.random.default_rng(2).standard_normal((30, 20)))
    r = _abi.svd_pca(_csc(A), 3, algorithm=4, nonneg=(True, True))
    assert r["status"] == -1 and "algorithm 0" in r["error"]


# ------------------------------------------------------------------------------------------------------------ surface routes
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def fake(name):
        def f(*a, **kw):
            seen.append((name, kw))
            return dict(status=-1, error="stub: " + name)
        return f
    for name in ("svd_pca", "svd_cv", "svd_krylov"):
        monkeypatch.setattr(_abi, name, fake(name))
    return seen


def test_surface_routes(calls):
    A = np.abs(np.random.default_rng(2).standard_normal((30, 20)))
    with pytest.raises(_abi.BackendError, match="stub: svd_krylov"):
        S.svd(A, k=10, nonneg=True, method="krylov")
    assert calls[-1][0] == "svd_krylov" and calls[-1][1]["max_iter"] == 0          # maxit missing: the default pass count
    with pytest.raises(_abi.BackendError, match="stub: svd_krylov"):
        S.svd(sp.csc_matrix(A), k=3, L1=0.1, method="krylov", maxit=7, precision="double")
    assert calls[-1][1]["max_iter"] == 7 and calls[-1][1]["precision"] == "double"
    n = len(calls)
    with pytest.raises(_abi.BackendError) as e:                                     # auto -> krylov: still refused, both ways named
        S.svd(A, k=10, nonneg=True)
    assert 'method = "krylov"' in str(e.value) and 'method = "deflation"' in str(e.value) and len(calls) == n
    with pytest.raises(_abi.BackendError, match="stub: svd_pca"):                   # unconstrained krylov: Lanczos, the reference entry
        S.svd(A, k=10, method="krylov")
    assert calls[-1][1]["algorithm"] == 4
    with pytest.raises(_abi.BackendError, match="need method 'deflation'"):         # krylov under CV or a mask: refused
        S.svd(A, k=10, nonneg=True, method="krylov", test_fraction=0.1)
    with pytest.raises(_abi.BackendError, match="need method 'deflation'"):
        S.svd(A, k=10, nonneg=True, method="krylov", mask=sp.random(30, 20, density=0.1, format="csc", random_state=1))
    with pytest.raises(_abi.BackendError, match="stub: svd_pca"):                   # auto below k = 8: deflation, as before
        S.svd(A, k=5, nonneg=True)
    assert calls[-1][1]["algorithm"] == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    A = np.abs(np.random.default_rng(2).standard_normal((30, 20)))
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        S.svd(A, k=10, nonneg=True, method="krylov")
