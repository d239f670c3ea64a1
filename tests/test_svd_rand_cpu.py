"""CPU checks of the randomized block SVD: the numpy restatement (tests/svd_rand_ref.py, the GPU path's parity target) on its own,
the ABI declarations and the refusals that hold before any device work, and the routes of svd().  No GPU needed."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import svd_rand_ref as RR
from rcppml_amd import _abi, svd as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ground_truth():
    """The reference's GPU SVD case (tests/testthat/test_gpu_svd.R:13-21): 30 x 20, singular values 50, 30, 15, 8, 4."""
    rng = np.random.default_rng(123)
    Uq, _ = np.linalg.qr(rng.standard_normal((30, 5)))
    Vq, _ = np.linalg.qr(rng.standard_normal((20, 5)))
    return (Uq * np.array([50.0, 30, 15, 8, 4])) @ Vq.T


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_sizes():
    assert RR.sizes(30, 20, 5) == (10, 15, 3)
    assert RR.sizes(30, 20, 15) == (5, 20, 3)
    assert RR.sizes(30, 20, 20) == (0, 20, 3)
    assert RR.sizes(30, 20, 5, 25)[2] == 10 and RR.sizes(30, 20, 5, 1)[2] == 1 and RR.sizes(30, 20, 5, -4)[2] == 3
    assert RR.sizes(3867, 610, 107)[:2] == (21, 128) and RR.sizes(3867, 610, 64)[:2] == (12, 76)
    for a in ((30, 20, 5), (30, 20, 15), (30, 20, 20), (30, 20, 5, 25), (3867, 610, 107), (183, 1183, 40, 2)):
        assert _abi.randomized_sizes(*a) == RR.sizes(*a)


def _draws(seed, count):
    """SplitMix64 by hand on Python integers: the 64-bit outputs of draws 0 .. count - 1."""
    M, state, out = (1 << 64) - 1, seed, []
    for _ in range(count):
        state = (state + 0x9E3779B97F4A7C15) & M
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        out.append(z ^ (z >> 31))
    return out


def test_splitmix_known_outputs():
    # the published SplitMix64 test vector for seed 1234567
    assert _draws(1234567, 3) == [6457827717110365317, 3203168211198807973, 9817491932198370423]


@pytest.mark.parametrize("seed", [0, 7])
def test_omega_against_hand_computed_draws(seed):
    n, l = 5, 3
    z = _draws(42 if seed == 0 else seed, n * l)
    for dt in (np.float64, np.float32):
        Om = RR.omega(n, l, seed, dt)
        assert Om.dtype == dt and Om.shape == (n, l)
        for j in range(l):
            for i in range(n):
                want = dt(z[j * n + i]) / dt(2.0 ** 64) - dt(0.5)          # column-major: draw j n + i
                assert Om[i, j] == want, (i, j)
        assert np.all(Om >= -0.5) and np.all(Om <= 0.5)
    assert np.array_equal(RR.splitmix_uniform(42, 4, 6), RR.splitmix_uniform(42, 0, 10)[4:])     # a pure function of the index


def test_restatement_on_the_rank_5_ground_truth():
    A = ground_truth()
    U0, s0, Vt0 = np.linalg.svd(A)
    r = RR.randomized_svd(A, 5)
    assert (r["p"], r["l"], r["q"]) == (10, 15, 3) and r["iters"].tolist() == [3]
    assert np.max(np.abs(r["d"] - s0[:5])) <= 1e-12 * s0[0]
    u, v = RR.align(U0[:, :5], r["u"], r["v"])
    assert np.max(np.abs(u - U0[:, :5])) <= 1e-12 and np.max(np.abs(v - Vt0[:5].T)) <= 1e-12
    for k in (15, 20):
        r = RR.randomized_svd(A, k, center=True)
        D = A - A.mean(axis=1, keepdims=True)
        assert r["d"].size == k and np.max(np.abs(r["d"][:5] - np.linalg.svd(D, compute_uv=False)[:5])) <= 1e-12 * s0[0]
        assert abs(r["frob"] - np.sum(D * D)) <= 1e-12 * np.sum(D * D)


# ------------------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entries_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_svd_randomized_ex", 38), ("rcppml_gpu_svd_randomized_dense_ex", 35)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert m.group(1).count("*") == count and len(m.group(1).split(",")) == count, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name), name
    assert "randomized.hpp" in src


def _csc(A):
    M = sp.csc_matrix(A)
    M.sort_indices()
    return (M.indptr, M.indices, M.data, A.shape[0], A.shape[1])


REFUSALS = [
    (dict(k=0), "k_max must be in [1, min(m, n)]"),
    (dict(k=21), "k_max must be in [1, min(m, n)]"),
    (dict(L1=(0.1, 0)), "the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)"),
    (dict(L2=(0, 0.1)), "the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)"),
    (dict(nonneg=(True, False)), "the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)"),
    (dict(upper_bound=(0, 1.0)), "the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)"),
    (dict(L21=(0.1, 0)), "the randomized method does not support L21"),
    (dict(angular=(0, 0.1)), "the randomized method does not support angular"),
    (dict(graph_u=([0] * 31, 0.5)), "the randomized method does not support graph regularization"),
    (dict(graph_v=([0] * 21, 0.5)), "the randomized method does not support graph regularization"),
    (dict(test_fraction=0.05), "the randomized method does not support test_fraction > 0 (cross-validation / auto-rank)"),
    (dict(obs_mask=[0] * 21), "the randomized method does not support obs_mask"),
    (dict(nan=True), "the matrix holds a non-finite value"),
]


def refusal_case(kw, dense, precision):
    """One refused call on pre-filled buffers: (result, buffers).  Shared with tests/test_gpu_svd_rand.py."""
    A = np.abs(np.random.default_rng(2).standard_normal((30, 20)))
    kw = dict(kw)
    k = kw.pop("k", 3)
    kb = max(k, 1)
    if kw.pop("nan", False):
        A[4, 6] = np.nan
    bufs = dict(U=np.full(30 * kb, 7.0), d=np.full(kb, 7.0), V=np.full(20 * kb, 7.0), row_means=np.full(30, 7.0),
                iters=np.full(kb, 7, np.int32))
    return _abi.svd_randomized(A if dense else _csc(A), k, dense=dense, precision=precision, center=True, buffers=bufs, **kw), bufs


@pytest.mark.parametrize("kw, msg", REFUSALS)
def test_abi_refusals_leave_buffers_untouched(kw, msg):
    """Refused before any device work, so these hold with or without a GPU."""
    for dense in (False, True):
        for precision in ("double", "float"):
            r, bufs = refusal_case(kw, dense, precision)
            assert (r["status"], r["error"]) == (-1, msg)
            assert all(np.all(b == 7) for b in bufs.values())
            assert (r["k"], r["frob"], r["wall_ms"]) == (0, 0.0, 0.0)


def test_abi_refuses_a_sketch_above_128_and_a_malformed_csc():
    A = sp.random(140, 135, density=0.2, format="csc", random_state=1)
    r = _abi.svd_randomized(_csc(A.toarray()), 108)                 # p = 21, l = 129
    assert (r["status"], r["error"]) == (-1, "the randomized method's sketch dimension l = k + oversampling = 129 is above the limit of 128")
    r = _abi.svd_randomized(A.toarray(), 130, dense=True)           # p = 5 (clamped), l = 135
    assert r["status"] == -1 and "l = k + oversampling = 135" in r["error"] and "128" in r["error"]
    x = np.array([1.0, 2.0, 3.0])
    for p, i, msg in (([1, 2, 3], [0, 2, 1], "col_ptr must start at 0 and end at nnz"), ([0, 4, 3], [0, 2, 1], "col_ptr must be non-decreasing"),
                      ([0, 2, 3], [0, 3, 1], "row index out of range")):
        r = _abi.svd_randomized((p, i, x, 3, 2), 1)
        assert (r["status"], r["error"]) == (-1, msg)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    A = ground_truth()
    r = _abi.svd_randomized(_csc(A), 5)
    assert (r["status"], r["error"]) == (-1, "no HIP device")
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        S.svd(A, k=5, method="randomized")


# ------------------------------------------------------------------------------------------------------------ surface routes
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def fake(name):
        def f(*a, **kw):
            seen.append((name, a, kw))
            return dict(status=-1, error="stub: " + name)
        return f
    for name in ("svd_pca", "svd_cv", "svd_krylov", "svd_randomized"):
        monkeypatch.setattr(_abi, name, fake(name))
    return seen


def test_surface_routes(calls):
    A = np.abs(np.random.default_rng(2).standard_normal((70, 80)))
    with pytest.raises(_abi.BackendError, match="stub: svd_randomized"):
        S.svd(A, k=10, method="randomized")
    assert calls[-1][2]["max_iter"] == 3 and calls[-1][2]["precision"] == "float" and calls[-1][2]["dense"] is True
    with pytest.raises(_abi.BackendError, match="stub: svd_randomized"):
        S.pca(sp.csc_matrix(A), k=4, method="randomized", maxit=25, precision="double", seed=9)
    kw = calls[-1][2]
    assert (kw["max_iter"], kw["precision"], kw["center"], kw["seed"], kw["dense"]) == (25, "double", True, 9, False)
    with pytest.raises(_abi.BackendError, match="stub: svd_pca"):                   # auto at 32 <= k < 64: R's randomized, Lanczos here
        S.pca(A, k=40)
    assert calls[-1][2]["algorithm"] == 3 and calls[-1][2]["max_iter"] == 3
    with pytest.raises(ValueError, match="method 'randomized' does not support constraints"):
        S.svd(A, k=4, method="randomized", nonneg=True)
    with pytest.raises(ValueError, match="method 'randomized' does not support auto-rank"):
        S.svd(A, k="auto", method="randomized")
    with pytest.raises(_abi.BackendError, match="need method 'deflation'"):         # a mask matrix: deflation only
        S.svd(A, k=4, method="randomized", mask=sp.random(70, 80, density=0.1, format="csc", random_state=1))
