"""GPU truncated SVD / PCA (rcppml_amd/csrc/ops_svd.hip) through the R-shaped C ABI: the reference's GPU SVD cases
(tests/testthat/test_gpu_svd.R), deflation against the numpy restatement of the reference's CPU path (tests/svd_ref.py), and
Lanczos against numpy's dense SVD."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_ref as R
from rcppml_amd import _abi, svd as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def fixture(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    A.sort_indices()
    return A


def parts(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def ground_truth():
    """test_gpu_svd.R:13-21: 30 x 20, singular values 50, 30, 15, 8, 4."""
    rng = np.random.default_rng(123)
    Uq, _ = np.linalg.qr(rng.standard_normal((30, 5)))
    Vq, _ = np.linalg.qr(rng.standard_normal((20, 5)))
    return (Uq * np.array([50.0, 30, 15, 8, 4])) @ Vq.T


def rel_recon(A, r):
    k = r["k"]
    return np.linalg.norm(A - (r["U"][:, :k] * r["d"][:k]) @ r["V"][:, :k].T) / np.linalg.norm(A)


@pytest.mark.parametrize("dense, method", [(False, "deflation"), (False, "krylov"), (False, "lanczos"), (False, "irlba"),
                                           (False, "randomized"), (True, "deflation"), (True, "lanczos"), (True, "irlba"),
                                           (True, "randomized")])
def test_reference_cases(dense, method):
    A = ground_truth()
    ref = np.linalg.svd(A, compute_uv=False)[:5]
    # test_gpu_svd.R: tol = 1e-10, seed = 1, maxit = 500 for deflation and krylov (else R's per-method default)
    _, maxit, tol, _ = S.resolve_method(5, method, **(dict(maxit=500) if method in ("deflation", "krylov") else {}), tol=1e-10)
    # R's .gpu_svd_pca uses the float entry by default; the dense path always calls the dense float entry
    r = _abi.svd_pca(A if dense else parts(A), 5, dense=dense, precision="float", tol=tol, max_iter=maxit, seed=1,
                     algorithm=_abi.SVD_ALGORITHMS[method])
    assert r["status"] == 0, r["error"]
    assert r["k"] == 5
    assert np.max(np.abs(r["d"][:5] - ref) / ref) < 1e-3
    assert rel_recon(A, r) < 1e-3


CONSTRAINTS = [dict(), dict(nonneg=(True, True)), dict(L1=(0.02, 0.02)), dict(upper_bound=(0.3, 0.3))]


@pytest.mark.parametrize("name", ["hawaiibirds", "movielens"])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("ci", range(len(CONSTRAINTS)))
def test_deflation_matches_restatement(name, center, ci):
    A = fixture(name)
    c = CONSTRAINTS[ci]
    k = 4
    ref = R.deflation_svd(A.toarray(), k, tol=1e-5, maxit=100, center=center, seed=0, **{("ub" if kk == "upper_bound" else kk): v
                                                                                             for kk, v in c.items()})
    r = _abi.svd_pca(parts(A), k, precision="double", tol=1e-5, max_iter=100, center=center, seed=0, algorithm=0, **c)
    assert r["status"] == 0, r["error"]
    ks = len(ref["d"])
    assert r["k"] == ks
    assert np.array_equal(r["iters"][:ks], ref["iters"])
    for a, b in ((r["U"][:, :ks], ref["u"]), (r["d"][:ks], ref["d"]), (r["V"][:, :ks], ref["v"])):
        assert np.max(np.abs(a - b)) <= 1e-10 * max(np.max(np.abs(b)), 1e-300)
    if center:
        assert np.allclose(r["row_means"], ref["row_means"], rtol=1e-12, atol=0)
    assert abs(r["frob"] - ref["frob"]) <= 1e-12 * abs(ref["frob"])
    rf = _abi.svd_pca(parts(A), k, precision="float", tol=1e-5, max_iter=100, center=center, seed=0, algorithm=0, **c)
    assert rf["status"] == 0, rf["error"]
    kf = min(rf["k"], ks)
    assert np.max(np.abs(rf["d"][:kf] - ref["d"][:kf])) <= 1e-4 * ref["d"][0]


def dense_ref(A, center):
    D = A.toarray()
    if center:
        D = D - D.mean(axis=1, keepdims=True)
    return D, np.linalg.svd(D, compute_uv=False)


@pytest.mark.parametrize("name", ["hawaiibirds", "movielens"])
@pytest.mark.parametrize("k", [1, 5, 31, 64])
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("center", [False, True])
def test_lanczos_against_numpy(name, k, dense, center):
    A = fixture(name)
    D, sv = dense_ref(A, center)
    src = A.toarray() if dense else parts(A)
    for prec, tol, lim in (("double", 1e-12, 1e-8), ("float", 1e-6, 1e-4)):
        # max_iter above the default 3k step cap: movielens' close pairs need more steps to converge at k = 31
        r = _abi.svd_pca(src, k, dense=dense, precision=prec, tol=tol, max_iter=300, center=center, seed=0, algorithm=2)
        assert r["status"] == 0, r["error"]
        assert r["k"] == k
        d = r["d"][:k]
        # every Ritz value sits on a true singular value; of a very close pair Lanczos may hold the lower one when its residual
        # test stops (movielens has such pairs), so the ordered comparison is to 1e-4 only
        near = np.min(np.abs(d[:, None] - sv[None, :]) / sv[None, :], axis=1)
        assert np.max(near) < lim, (prec, np.max(near))
        assert np.max(np.abs(d - sv[:k]) / sv[:k]) < 1e-4
        U, V = r["U"][:, :k], r["V"][:, :k]
        olim = 1e-8 if prec == "double" else 1e-4
        assert np.max(np.abs(U.T @ U - np.eye(k))) < olim and np.max(np.abs(V.T @ V - np.eye(k))) < olim
        assert r["iters"][0] >= k
        if center:
            assert np.allclose(r["row_means"], A.toarray().mean(axis=1), rtol=1e-12, atol=1e-300)
        assert abs(r["frob"] - np.sum(D * D)) <= 1e-10 * np.sum(D * D)


def test_empty_rows_columns_and_full_rank():
    A = ground_truth()
    A = np.insert(A, 7, 0.0, axis=0)          # an empty row
    A = np.insert(A, 3, 0.0, axis=1)          # an empty column
    m, n = A.shape
    sv = np.linalg.svd(A, compute_uv=False)
    for alg in (0, 2):
        r = _abi.svd_pca(parts(A), min(m, n), precision="double", tol=1e-10, max_iter=500, seed=3, algorithm=alg)
        assert r["status"] == 0, r["error"]
        assert 5 <= r["k"] <= min(m, n)
        assert np.max(np.abs(r["d"][:5] - sv[:5]) / sv[:5]) < 1e-6
        assert rel_recon(A, r) < 1e-4                    # deflation's vectors are good to ~ sqrt(tol)
    r = _abi.svd_pca(parts(A), 5, precision="double", tol=1e-10, max_iter=0, algorithm=2)
    rd = _abi.svd_pca(A, 5, dense=True, precision="double", tol=1e-10, max_iter=0, algorithm=2)
    assert r["status"] == 0 and rd["status"] == 0
    assert np.max(np.abs(r["d"][:5] - rd["d"][:5]) / sv[:5]) < 1e-10


def test_refused_cases_leave_buffers_untouched_on_the_device():
    A = fixture("hawaiibirds")
    for kw in (dict(test_fraction=0.05), dict(algorithm=2, nonneg=(True, False)), dict(robust_delta=1.0), dict(L21=(0.0, 0.1))):
        bufs = dict(U=np.full(183 * 3, 7.0), d=np.full(3, 7.0), V=np.full(1183 * 3, 7.0), row_means=np.full(183, 7.0),
                    iters=np.full(3, 7, np.int32))
        r = _abi.svd_pca(parts(A), 3, center=True, buffers=bufs, **kw)
        assert r["status"] == -1 and r["error"]
        assert all(np.all(b == 7) for b in bufs.values())


@pytest.mark.parametrize("alg, prec", [(0, "double"), (0, "float"), (2, "double"), (2, "float")])
def test_two_runs_are_bitwise_identical(alg, prec):
    A = fixture("movielens")
    a = _abi.svd_pca(parts(A), 6, precision=prec, center=True, algorithm=alg, max_iter=100 if alg == 0 else 0)
    b = _abi.svd_pca(parts(A), 6, precision=prec, center=True, algorithm=alg, max_iter=100 if alg == 0 else 0)
    assert a["status"] == 0 and b["status"] == 0
    for key in ("U", "V", "d", "iters"):
        assert np.array_equal(a[key], b[key]), key


def test_python_surface():
    A = fixture("hawaiibirds")
    r = S.pca(A, k=5, precision="double", tol=1e-10)
    assert r["misc"]["method"] == "lanczos"
    D, sv = dense_ref(A, True)
    assert np.max(np.abs(r["d"] - sv[:5]) / sv[:5]) < 1e-8
    assert np.allclose(r["misc"]["row_means"], A.toarray().mean(axis=1))
    r = S.svd(A, k=3, nonneg=True, precision="double")
    assert r["misc"]["method"] == "deflation" and len(r["misc"]["iters_per_factor"]) == r["d"].size
    assert np.all(r["u"][:, 0] >= 0) and np.all(r["v"][:, 0] >= 0)   # later factors: Gram-Schmidt may leave negatives
    with pytest.raises(_abi.BackendError):
        S.svd(A, k=10, nonneg=True)                       # R resolves this to krylov, which the GPU refuses with constraints
