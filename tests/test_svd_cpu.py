"""CPU checks of the truncated SVD / PCA feature: the numpy restatement of the reference's CPU deflation SVD (tests/svd_ref.py, the
GPU path's parity target), the ABI declarations and exports, R's method resolution and messages, and the refusals that hold
before any device work.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import svd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("rcppml_gpu_svd_pca_double", 61), ("rcppml_gpu_svd_pca_float", 61), ("rcppml_gpu_svd_pca_dense_double", 58),
           ("rcppml_gpu_svd_pca_dense_float", 58))


def known_30x20(sig=(50.0, 30.0, 15.0, 8.0, 4.0), seed=7):
    rng = np.random.default_rng(seed)
    Uq, _ = np.linalg.qr(rng.standard_normal((30, len(sig))))
    Vq, _ = np.linalg.qr(rng.standard_normal((20, len(sig))))
    return (Uq * np.asarray(sig)) @ Vq.T, np.asarray(sig)


def test_header_declares_the_reference_pointer_lists():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name, count in ENTRIES:
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        args = m.group(1)
        assert args.count("*") == count and len(args.split(",")) == count, name


def test_library_exports_the_entries():
    from rcppml_amd import _abi
    L = _abi.lib()
    for name, _ in ENTRIES:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_restatement_recovers_known_singular_values():
    A, sig = known_30x20()
    r = R.deflation_svd(A, 5, tol=1e-12, maxit=2000)
    ref = np.linalg.svd(A, compute_uv=False)[:5]
    assert np.allclose(ref, sig, rtol=1e-12)
    assert np.max(np.abs(r["d"] - sig) / sig) < 1e-8
    assert np.allclose(r["u"].T @ r["u"], np.eye(5), atol=1e-8)
    assert np.allclose((r["u"] * r["d"]) @ r["v"].T, A, atol=1e-4 * sig[0])
    assert np.all(r["iters"] >= 1)


def test_restatement_centering_and_norm():
    A, _ = known_30x20()
    A = A + 3.0
    r = R.deflation_svd(A, 3, tol=1e-12, maxit=2000, center=True)
    Ac = A - A.mean(axis=1, keepdims=True)
    assert np.allclose(r["row_means"], A.mean(axis=1))
    assert abs(r["frob"] - np.sum(Ac * Ac)) < 1e-9 * np.sum(Ac * Ac)
    assert np.max(np.abs(r["d"] - np.linalg.svd(Ac, compute_uv=False)[:3]) / r["d"]) < 1e-8


def test_restatement_start_is_splitmix_seed_42():
    from rcppml_amd.data import splitmix64_uniform
    A, _ = known_30x20()
    one = R.deflation_svd(A, 1, maxit=1, seed=0)
    same = R.deflation_svd(A, 1, maxit=1, seed=42)
    assert np.array_equal(one["u"], same["u"])
    u0 = splitmix64_uniform(42, 0, 30)
    assert np.all(u0 > 0) and np.all(u0 < 1)


def test_method_resolution_is_rs():
    from rcppml_amd.svd import resolve_method
    assert resolve_method(5)[:2] == ("lanczos", 0)
    assert resolve_method(40)[:2] == ("randomized", 3)
    assert resolve_method(64)[:2] == ("irlba", 0)
    assert resolve_method(5, nonneg=True)[:2] == ("deflation", 200)
    assert resolve_method(8, L1=0.1)[:2] == ("krylov", 0)
    assert resolve_method(5, method="deflation")[:2] == ("deflation", 200)
    assert resolve_method(5, method="lanczos", maxit=50)[:2] == ("lanczos", 50)
    assert resolve_method(5, maxit=30)[:2] == ("lanczos", 30)


@pytest.mark.parametrize("kw, msg", [
    (dict(method="qr"), "method must be one of: auto, deflation, krylov, lanczos, irlba, randomized"),
    (dict(k=0), "'k' must be >= 1"),
    (dict(L1=-1), "L1 penalties must be non-negative"),
    (dict(L2=-1), "L2 penalties must be non-negative"),
    (dict(upper_bound=-1), "upper_bound must be non-negative"),
    (dict(tol=-1), "'tol' must be non-negative"),
    (dict(method="deflation", maxit=0), "'maxit' must be >= 1"),
    (dict(method="lanczos", nonneg=True),
     "method 'lanczos' does not support constraints (L1/L2/nonneg/bounds/L21). Use 'deflation' or 'krylov'."),
    (dict(method="irlba", L1=0.5),
     "method 'irlba' does not support constraints (L1/L2/nonneg/bounds/L21). Use 'deflation' or 'krylov'."),
])
def test_validation_messages_are_rs(kw, msg):
    from rcppml_amd.svd import resolve_method
    kw = dict(kw)
    k = kw.pop("k", 5)
    with pytest.raises(ValueError) as e:
        resolve_method(k, **kw)
    assert str(e.value) == msg


def _csc(A):
    import scipy.sparse as sp
    S = sp.csc_matrix(A)
    S.sort_indices()
    return (S.indptr, S.indices, S.data, A.shape[0], A.shape[1])


@pytest.mark.parametrize("kw", [dict(test_fraction=0.1), dict(L21=(0.1, 0)), dict(angular=(0, 0.1)), dict(robust_delta=1.345),
                                dict(algorithm=2, nonneg=(True, True)), dict(algorithm=4, L1=(0.1, 0)), dict(algorithm=7),
                                dict(k=0), dict(k=21), dict(max_iter=0)])
def test_abi_refusals_leave_buffers_untouched(kw):
    """Refused before any device work, so these hold with or without a GPU."""
    from rcppml_amd import _abi
    A, _ = known_30x20()
    kw = dict(kw)
    k = kw.pop("k", 3)
    kb = max(k, 1)
    bufs = dict(U=np.full(30 * kb, 7.0), d=np.full(kb, 7.0), V=np.full(20 * kb, 7.0), row_means=np.full(30, 7.0),
                iters=np.full(kb, 7, np.int32))
    r = _abi.svd_pca(_csc(A), k, buffers=bufs, **kw)
    assert r["status"] == -1 and r["error"]
    for b in bufs.values():
        assert np.all(b == 7)
    r = _abi.svd_pca(A, k, dense=True, precision="float", buffers=bufs, **kw)
    assert r["status"] == -1 and r["error"]


# a 3 x 2 matrix (p = [0, 2, 3], i = [0, 2, 1]) with one defect each; nnz is the length of x
@pytest.mark.parametrize("p, i, k, msg", [
    ([1, 2, 3], [0, 2, 1], 1, "col_ptr must start at 0 and end at nnz"),
    ([0, 4, 3], [0, 2, 1], 1, "col_ptr must be non-decreasing"),
    ([0, 2, 3], [0, 3, 1], 1, "row index out of range"),
    ([0, 2, 3], [0, 2, 1], 0, "k_max must be in [1, min(m, n)]"),
])
@pytest.mark.parametrize("precision", ["double", "float"])
def test_malformed_input_refusals_are_exact(p, i, k, msg, precision):
    """Refused before any device work (so with or without a GPU): status -1, this message, nothing written."""
    from rcppml_amd import _abi
    x = np.array([1.0, 2.0, 3.0])
    bufs = dict(U=np.full(3, 7.0), d=np.full(1, 7.0), V=np.full(2, 7.0), row_means=np.full(3, 7.0), iters=np.full(1, 7, np.int32),
                test_loss=np.full(1, 7.0))
    r = _abi.svd_pca((p, i, x, 3, 2), k, precision=precision, center=True, buffers=bufs)
    assert (r["status"], r["error"]) == (-1, msg)
    assert all(np.all(b == 7) for b in bufs.values())
    assert (r["k"], r["frob"], r["wall_ms"]) == (0, 0.0, 0.0)


def test_abi_refuses_obs_mask_and_graph():
    from rcppml_amd import _abi
    A, _ = known_30x20()
    p, i, x, m, n = _csc(A)
    r = _abi.svd_pca(_csc(A), 3, obs_mask=(p, i, x, m, n))
    assert r["status"] == -1 and "obs_mask" in r["error"]
    g = _csc(np.eye(30))
    r = _abi.svd_pca(_csc(A), 3, graph_u=(g[0], g[1], g[2], 30, 0.5))
    assert r["status"] == -1 and "graph" in r["error"]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    from rcppml_amd import _abi, svd
    A, _ = known_30x20()
    with pytest.raises(_abi.BackendError):
        svd.pca(A, k=3)
