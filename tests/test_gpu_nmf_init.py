"""The SVD-seeded NMF start on the device (rcppml_gpu_nmf_svd_init_ex / _dense_ex, nmf_start_kernel) and nmf(seed = "lanczos" |
"irlba"): against LAPACK, bitwise against the Ritz path of rcppml_gpu_svd_pca_* transformed on the host, the fill rows against
tests/nmf_init_ref.py, and nmf() with a string seed against the same fit started from the entry's two arrays."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import nmf_init_ref as IR
from rcppml_amd import _abi, nmf as N

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 32                                   # NS_CW of kernels_svd.hip.h: columns a thread accumulates in one walk of the basis
RANKS = (5, CHUNK + 1)
LIMIT = {"double": 1e-8, "float": 1e-4}      # the limits test_lanczos_against_numpy sets for this engine's vectors
DT = {"double": np.float64, "float": np.float32}


def spectrum_matrix(m, n, seed=11):
    """A = (Q_U s) Q_V': s_c = 0.8^c for c < 40, then a tail 1e-5 0.97^c."""
    rng = np.random.default_rng(seed)
    r = min(m, n)
    qu, _ = np.linalg.qr(rng.standard_normal((m, r)))
    qv, _ = np.linalg.qr(rng.standard_normal((n, r)))
    c = np.arange(r, dtype=np.float64)
    return (qu * np.where(c < 40, 0.8 ** c, 1e-5 * 0.97 ** c)) @ qv.T


def parts(A):
    """every entry stored, column by column: the full CSC of a dense matrix"""
    m, n = A.shape
    return (np.arange(n + 1, dtype=np.int32) * m, np.tile(np.arange(m, dtype=np.int32), n), np.ascontiguousarray(A.ravel(order="F")), m, n)


MATS = {"197x131": spectrum_matrix(197, 131)}
MATS["131x197"] = np.ascontiguousarray(MATS["197x131"].T)
SVDS = {key: np.linalg.svd(A, full_matrices=False) for key, A in MATS.items()}


def start(A, k, dense, precision, seed=3, mode=1, **kw):
    r = _abi.nmf_svd_init(A if dense else parts(A), k, dense=dense, precision=precision, seed=seed, mode=mode, **kw)
    assert r["status"] == 0, r["error"]
    return r


def lapack_gap(r, usv, ks):
    """max |difference| of the first ks rows of W_T and H to |u| sqrt(s), |v| sqrt(s), relative to the factor's largest entry"""
    u, s, vt = usv
    out = []
    for got, vec in ((r["W_T"], u[:, :ks]), (r["H"], vt[:ks].T)):
        ref = np.abs(vec) * np.sqrt(s[:ks])
        out.append(np.max(np.abs(got[:, :ks] - ref)) / np.max(np.abs(ref)))
    return max(out)


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("key", list(MATS))
def test_start_against_lapack(key, k, dense, precision):
    """Measured on an MI355X: fp64 at most 2.8e-15 at k = 5 and 8.9e-12 at k = 33, fp32 at most 2.5e-7 and 7.9e-7."""
    r = start(MATS[key], k, dense, precision)
    assert r["k_svd"] == k and 0 < r["iters"] <= max(3 * k, k + 50)
    gap = lapack_gap(r, SVDS[key], k)
    dgap = np.max(np.abs(r["d"] - SVDS[key][1][:k])) / SVDS[key][1][0]
    print("%s k=%d %s %s: steps %d, factor gap %.3e, sigma gap %.3e" % (key, k, "dense" if dense else "csc", precision, r["iters"], gap, dgap))
    assert gap < LIMIT[precision] and dgap < LIMIT[precision]
    assert np.all(r["W_T"] >= 0) and np.all(r["H"] >= 0)


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("key", list(MATS))
def test_start_is_bitwise_the_ritz_path_transformed(key, k, dense, precision):
    """The same basis, the same sums in the same order: a condition, not a tolerance."""
    assert_start_is_the_ritz_path_transformed(MATS[key], k, dense, precision)


def assert_start_is_the_ritz_path_transformed(A, k, dense, precision):
    """Also what tests/test_gpu_svd_geometry.py asserts of its matrices, whose rows fill more than two blocks of nmf_start_kernel."""
    r = start(A, k, dense, precision, seed=5)
    s = _abi.svd_pca(A if dense else parts(A), k, dense=dense, precision=precision, algorithm=2, tol=1e-10, max_iter=0, seed=5)
    assert s["status"] == 0, s["error"]
    assert s["k"] == r["k_svd"] == k and s["iters"][0] == r["iters"]
    dt = DT[precision]
    sq = np.sqrt(s["d"][:k].astype(dt))
    assert np.array_equal(r["d"], s["d"][:k])
    assert np.array_equal(r["W_T"], (np.abs(s["U"].astype(dt)) * sq).astype(np.float64))
    assert np.array_equal(r["H"], (np.abs(s["V"].astype(dt)) * sq).astype(np.float64))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
def test_rank_deficient_input_fills_the_missing_rows(dense, precision):
    rng = np.random.default_rng(4)
    m, n, k, seed = 70, 45, 5, 12
    qu, _ = np.linalg.qr(rng.standard_normal((m, 3)))
    qv, _ = np.linalg.qr(rng.standard_normal((n, 3)))
    A = (qu * np.array([3.0, 2.0, 1.0])) @ qv.T             # the recipe of the other matrices, three singular values
    r = start(A, k, dense, precision, seed=seed)
    assert r["k_svd"] == 3 and r["d"].shape == (3,)
    usv = np.linalg.svd(A, full_matrices=False)
    gap = lapack_gap(r, usv, 3)
    print("rank 3, %s %s: steps %d, gap %.3e" % ("dense" if dense else "csc", precision, r["iters"], gap))
    assert gap < LIMIT[precision]
    W_ref, H_ref = IR.initialize_lanczos(usv[0][:, :3], usv[1][:3], usv[2][:3].T, k, m, n, seed, DT[precision])
    assert np.array_equal(r["W_T"][:, 3:], W_ref[:, 3:].astype(np.float64))
    assert np.array_equal(r["H"][:, 3:], H_ref[:, 3:].astype(np.float64))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
@pytest.mark.parametrize("shape, k", [((1, 9), 1), ((9, 1), 1), ((40, 23), 23), ((23, 40), 23)])
def test_edge_shapes_return_finite_values(shape, k, dense, precision):
    A = np.abs(np.random.default_rng(8).standard_normal(shape)) + 0.1
    r = start(A, k, dense, precision)
    assert 1 <= r["k_svd"] <= k
    assert np.all(np.isfinite(r["W_T"])) and np.all(np.isfinite(r["H"])) and np.all(np.isfinite(r["d"]))
    assert r["W_T"].shape == (shape[0], k) and r["H"].shape == (shape[1], k)
    if shape[1] <= k:
        # k steps from a start vector in R^n span all of R^n: the leading triplet is then exact up to rounding.  (With n > k the
        # space is k-dimensional and holds the start vector's null-space part: a 1 x 9 input gets one step and |A p_0| for sigma.)
        assert r["k_svd"] == k and lapack_gap(r, np.linalg.svd(A, full_matrices=False), 1) < LIMIT[precision]


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
def test_two_runs_are_bitwise_equal_and_mode_2_is_the_same_engine(dense, precision):
    A = MATS["131x197"]
    a, b, c = (start(A, CHUNK + 1, dense, precision, mode=mode) for mode in (1, 1, 2))
    for key in ("W_T", "H", "d"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key])
    assert a["iters"] == b["iters"] == c["iters"]


@pytest.mark.parametrize("dense", [False, True], ids=["csc", "dense"])
@pytest.mark.parametrize("k", [0, 132])
def test_refused_call_leaves_poisoned_buffers_untouched(k, dense):
    A = MATS["197x131"]
    for precision in ("double", "float"):
        bufs = dict(W_T=np.full(197 * 132, 7.0), H=np.full(131 * 132, 7.0), d=np.full(132, 7.0))
        r = _abi.nmf_svd_init(A if dense else parts(A), k, dense=dense, precision=precision, buffers=bufs)
        assert (r["status"], r["error"]) == (-1, "k_max must be in [1, min(m, n)]")
        assert all(np.all(b == 7) for b in bufs.values())
        assert (r["k_svd"], r["iters"], r["wall_ms"]) == (0, 0, 0.0)


# ----------------------------------------------------------------------------- nmf() with a string seed
def hawaiibirds():
    z = np.load(os.path.join(HERE, "golden", "hawaiibirds.npz"))
    A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    A.sort_indices()
    return A


def recorded(monkeypatch, name):
    """The calls nmf() makes of _abi.<name>, with the two factor arrays as they go in."""
    calls, real = [], getattr(_abi, name)

    def wrapper(*a, **kw):
        calls.append(([np.array(v, copy=True) if isinstance(v, np.ndarray) else v for v in a], dict(kw)))
        return real(*a, **kw)

    monkeypatch.setattr(_abi, name, wrapper)
    return calls, real


@pytest.mark.parametrize("path", ["plain", "cv", "dense"])
def test_string_seed_is_the_fit_started_from_the_entry_s_arrays(path, monkeypatch):
    """nmf(A, 6, seed = "lanczos", svd_seed = 7) against the same entry call -- every argument equal, the fit's seed included --
    started from the W_T and H of _abi.nmf_svd_init: bitwise the same w, d, h and iteration count."""
    S = hawaiibirds()
    data = S.toarray() if path == "dense" else S
    entry = {"plain": "nmf_unified", "cv": "nmf_cv", "dense": "nmf_dense"}[path]
    calls, real = recorded(monkeypatch, entry)
    kw = dict(test_fraction=0.1) if path == "cv" else {}
    mod = N.nmf(data, 6, seed="lanczos", svd_seed=7, precision="fp64", **kw)
    assert mod.misc["init"] == "lanczos" and mod.misc["init_k_svd"] == 6
    assert mod.misc["init_iters"] > 0 and mod.misc["init_wall_ms"] > 0 and mod.misc["seed"] == 7
    assert mod.misc.get("input") == ("dense" if path == "dense" else None)
    init = _abi.nmf_svd_init(data if path == "dense" else (S.indptr, S.indices, S.data, S.shape[0], S.shape[1]), 6,
                             dense=path == "dense", precision="double", seed=7, mode=1)
    assert init["status"] == 0 and init["k_svd"] == 6
    (args, kwargs), = calls
    wpos, hpos = (2, 3) if path == "dense" else (6, 7)        # nmf_dense(A, k, W_T, H, ...); the sparse wrappers (p, i, x, m, n, k, W_T, H, ...)
    assert np.array_equal(args[wpos], init["W_T"]) and np.array_equal(args[hpos], init["H"])
    W, H = init["W_T"].copy(), init["H"].copy()
    args[wpos], args[hpos] = W, H
    res = real(*args, **kwargs)
    assert res["status"] == 0, res.get("error")
    assert res["iter"] == mod.misc["iter"] and mod.misc["iter"] > 0
    assert np.array_equal(W, mod.w) and np.array_equal(H.T, mod.h) and np.array_equal(res["d"], mod.d)


def test_string_seed_through_the_public_surface():
    S = hawaiibirds()
    a = N.nmf(S, 6, seed="irlba", svd_seed=7, precision="fp32")
    b = N.nmf(S, 6, seed="svd", svd_seed=7, precision="fp32")
    assert a.misc["init"] == "irlba" and b.misc["init"] == "svd" and a.misc["init_k_svd"] == 6
    assert np.array_equal(a.w, b.w) and np.array_equal(a.h, b.h) and np.array_equal(a.d, b.d) and a.misc["iter"] == b.misc["iter"]
    assert np.all(np.isfinite(a.w)) and np.all(a.w >= 0) and np.all(a.h >= 0)
    c = N.nmf(S, 6, seed="random", precision="fp32", maxit=3)
    assert "init" not in c.misc
    rows = N.nmf(S, [3, 4], seed="lanczos", svd_seed=7, test_fraction=0.1, precision="fp32", maxit=10)
    assert rows.col("k") == [3, 4] and all(np.isfinite(v) for v in rows.col("test_mse"))
