"""GPU randomized block SVD (rcppml_gpu_svd_randomized_ex, rcppml_gpu_svd_randomized_dense_ex: rcppml_amd/csrc/ops_svd.hip,
kernels_svd_rand.hip.h) against the numpy restatement of the reference's CPU method (tests/svd_rand_ref.py), column signs aligned
by the sign of u_ref . u.

Bounds.  fp64: the device orthonormalises by CholeskyQR2 and takes the small SVD from the l x l Gram, the restatement uses
Householder QR and LAPACK's SVD; both are backward stable at the level eps d_1, a vector moves by eps d_1 / gap, and the smallest
relative gap among the parity cases is 3e-4, so 1e-12 d_1 for d and 1e-10 for vectors and orthogonality leave margin.  The wide
cases compare d and the rank-k product only (movielens has a relative gap of 2.7e-5 at k = 64).  fp32 is held to the 1e-4 d_1 the
other fp32 SVD tests use, against the float64 restatement."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_rand_ref as RR
from rcppml_amd import _abi, svd as S
from test_svd_rand_cpu import REFUSALS, ground_truth, refusal_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def dense_of(name):
    return fixture(name).toarray()


@functools.lru_cache(maxsize=None)
def reference(name, k, center, maxit=0):
    """The float64 restatement, computed once per case and shared (never modified)."""
    return RR.randomized_svd(dense_of(name), k, maxit=maxit, center=center)


def parts(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return (A.indptr, A.indices, A.data, A.shape[0], A.shape[1])


def run(name, k, dense=False, **kw):
    r = _abi.svd_randomized(dense_of(name) if dense else parts(fixture(name)), k, dense=dense, **kw)
    assert r["status"] == 0, r["error"]
    assert r["k"] == k
    return r


def product(u, d, v):
    return (u * d) @ v.T


def check_parity(r, ref, k, center, dlim, vlim):
    d1 = ref["d"][0]
    ed = np.max(np.abs(r["d"][:k] - ref["d"])) / d1
    u, v = RR.align(ref["u"], r["U"][:, :k], r["V"][:, :k])
    eu, ev = np.max(np.abs(u - ref["u"])), np.max(np.abs(v - ref["v"]))
    ou, ov = np.max(np.abs(u.T @ u - np.eye(k))), np.max(np.abs(v.T @ v - np.eye(k)))
    print("d %.3g  u %.3g  v %.3g  u'u %.3g  v'v %.3g" % (ed, eu, ev, ou, ov))
    assert ed <= dlim
    assert eu <= vlim and ev <= vlim
    assert ou <= vlim and ov <= vlim
    assert r["iters"][0] == ref["q"]
    assert abs(r["frob"] - ref["frob"]) <= 1e-12 * abs(ref["frob"])
    if center:
        assert np.allclose(r["row_means"], ref["row_means"], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("name", ["hawaiibirds", "movielens"])
@pytest.mark.parametrize("k", [4, 10, 40])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("dense", [False, True])
def test_parity_fp64(name, k, center, dense):
    ref = reference(name, k, center)
    assert ref["l"] == {4: 14, 10: 20, 40: 50}[k]
    check_parity(run(name, k, dense, precision="double", center=center), ref, k, center, 1e-12, 1e-10)


@pytest.mark.parametrize("k, l", [(64, 76), (107, 128)])
def test_wide_sketch_fp64(k, l):
    ref = reference("movielens", k, False)
    assert ref["l"] == l
    r = run("movielens", k, precision="double")
    ed = np.max(np.abs(r["d"][:k] - ref["d"])) / ref["d"][0]
    P, P0 = product(r["U"][:, :k], r["d"][:k], r["V"][:, :k]), product(ref["u"], ref["d"], ref["v"])
    ep = np.linalg.norm(P - P0) / np.linalg.norm(P0)
    print("d %.3g  product %.3g" % (ed, ep))
    assert ed <= 1e-12
    assert ep <= 1e-9


@pytest.mark.parametrize("name", ["hawaiibirds", "movielens"])
@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("dense", [False, True])
def test_fp32(name, k, center, dense):
    ref = reference(name, k, center)
    r = run(name, k, dense, precision="float", center=center)
    ed = np.max(np.abs(r["d"][:k] - ref["d"])) / ref["d"][0]
    u, v = r["U"][:, :k], r["V"][:, :k]
    P0 = product(ref["u"], ref["d"], ref["v"])
    ep = np.linalg.norm(product(u, r["d"][:k], v) - P0) / np.linalg.norm(P0)
    ou, ov = np.max(np.abs(u.T @ u - np.eye(k))), np.max(np.abs(v.T @ v - np.eye(k)))
    print("d %.3g  product %.3g  u'u %.3g  v'v %.3g" % (ed, ep, ou, ov))
    assert ed <= 1e-4
    assert ep <= 1e-4
    assert ou <= 1e-4 and ov <= 1e-4


def with_empty_row_and_column(A):
    return np.insert(np.insert(A, 7, 0.0, axis=0), 3, 0.0, axis=1)


@pytest.mark.parametrize("k", [5, 15, 20])
@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("dense", [False, True])
def test_rank_deficient_and_clamped(k, precision, empty, dense):
    """30 x 20 of rank 5: k = 5 has l = 15 (ten rejected pivots), k = 15 has p = 5, k = 20 has p = 0 and l = n (one more column with
    the empty row and column).  Beyond the rank the Gram eigenproblem resolves sqrt(eps) d_1 at best, so 1e-6 d_1 it is."""
    A = ground_truth()
    if empty:
        A = with_empty_row_and_column(A)
    sv = np.linalg.svd(A, compute_uv=False)
    r = _abi.svd_randomized(A if dense else parts(A), k, dense=dense, precision=precision)
    assert r["status"] == 0, r["error"]
    assert r["k"] == k and r["iters"][0] == 3
    d, U, V = r["d"][:k], r["U"][:, :k], r["V"][:, :k]
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(U)) and np.all(np.isfinite(V))
    print("d[:5] error %.3g  beyond the rank %.3g" % (np.max(np.abs(d[:5] - sv[:5])), np.max(d[5:], initial=0.0) / sv[0]))
    assert np.max(np.abs(d[:5] - sv[:5])) <= (1e-10 if precision == "double" else 1e-4 * sv[0])
    assert np.all(d[5:] <= 1e-6 * sv[0])
    assert np.all(np.diff(d) <= 0)
    P = product(U[:, :5], d[:5], V[:, :5])
    assert np.linalg.norm(P - A) <= (1e-10 if precision == "double" else 1e-4) * np.linalg.norm(A)


@pytest.mark.parametrize("max_iter, q", [(1, 1), (0, 3), (25, 10)])
def test_power_iterations(max_iter, q):
    ref = reference("hawaiibirds", 10, True, max_iter)
    assert ref["q"] == q
    r = run("hawaiibirds", 10, precision="double", center=True, max_iter=max_iter)
    assert r["iters"][0] == q and not r["iters"][1:].any()
    check_parity(r, ref, 10, True, 1e-12, 1e-10)


@pytest.mark.parametrize("precision", ["double", "float"])
def test_two_runs_are_bitwise_identical(precision):
    a = run("movielens", 10, precision=precision, center=True)
    b = run("movielens", 10, precision=precision, center=True)
    for key in ("U", "V", "d", "iters", "row_means"):
        assert np.array_equal(a[key], b[key]), key
    assert a["frob"] == b["frob"]
    c = run("movielens", 10, precision=precision, center=True, seed=5)
    assert not np.array_equal(a["U"], c["U"])                      # the seed reaches the sketch


@pytest.mark.parametrize("kw, msg", REFUSALS)
def test_refusals_leave_buffers_untouched_on_the_device(kw, msg):
    for dense in (False, True):
        r, bufs = refusal_case(kw, dense, "double")
        assert (r["status"], r["error"]) == (-1, msg)
        assert all(np.all(b == 7) for b in bufs.values())


def test_refusals_of_size_pointers_and_memory():
    A = sp.random(140, 135, density=0.2, format="csc", random_state=1)
    bufs = dict(U=np.full(140 * 108, 7.0), d=np.full(108, 7.0), V=np.full(135 * 108, 7.0), row_means=np.full(140, 7.0),
                iters=np.full(108, 7, np.int32))
    r = _abi.svd_randomized(parts(A), 108, center=True, buffers=bufs)
    assert (r["status"], r["error"]) == (-1, "the randomized method's sketch dimension l = k + oversampling = 129 is above the limit of 128")
    assert all(np.all(b == 7) for b in bufs.values())
    x = np.array([1.0, 2.0, 3.0])
    for p, i, msg in (([1, 2, 3], [0, 2, 1], "col_ptr must start at 0 and end at nnz"), ([0, 4, 3], [0, 2, 1], "col_ptr must be non-decreasing"),
                      ([0, 2, 3], [0, 3, 1], "row index out of range")):
        bufs = dict(U=np.full(3, 7.0), d=np.full(1, 7.0), V=np.full(2, 7.0), row_means=np.full(3, 7.0), iters=np.full(1, 7, np.int32))
        r = _abi.svd_randomized((p, i, x, 3, 2), 1, center=True, buffers=bufs)
        assert (r["status"], r["error"]) == (-1, msg)
        assert all(np.all(b == 7) for b in bufs.values())
    st = C.c_int(-99)
    _abi.lib().rcppml_gpu_svd_randomized_ex(*([None] * 37 + [C.byref(st)]))
    assert st.value == -1 and _abi.last_error() == "null pointer"
    _abi.lib().rcppml_gpu_svd_randomized_dense_ex(*([None] * 34 + [C.byref(st)]))
    assert st.value == -1 and _abi.last_error() == "null pointer"
    # the memory guard: two thousand million rows of which three hold a value; the entry sizes its blocks before it allocates any
    m = 2_000_000_000
    bufs = dict(U=np.full(8, 7.0), d=np.full(5, 7.0), V=np.full(8, 7.0), row_means=np.full(8, 7.0), iters=np.full(5, 7, np.int32))
    p = np.array([0, 1, 2, 3] + [3] * 17, np.int32)
    r = _abi.svd_randomized((p, np.array([0, 5, m - 1], np.int32), x, m, 20), 5, center=True, buffers=bufs)
    assert r["status"] == -1
    assert r["error"].startswith("the SVD needs ") and " bytes of device memory, " in r["error"]
    assert int(r["error"].split()[3]) > 400e9
    assert all(np.all(b == 7) for b in bufs.values())


def test_python_surface():
    for name in ("hawaiibirds", "movielens"):
        A = fixture(name)
        ref = reference(name, 10, False)
        r = S.svd(A, k=10, method="randomized", precision="double")
        mi = r["misc"]
        assert mi["method"] == "randomized" and mi["iters_per_factor"].tolist() == [3] and mi["k_selected"] == 10
        assert r["u"].shape == (A.shape[0], 10) and r["v"].shape == (A.shape[1], 10)
        assert np.max(np.abs(r["d"] - ref["d"])) <= 1e-12 * ref["d"][0]
        u, v = RR.align(ref["u"], r["u"], r["v"])
        assert np.max(np.abs(u - ref["u"])) <= 1e-10 and np.max(np.abs(v - ref["v"])) <= 1e-10
    A = fixture("hawaiibirds")
    rp = S.pca(A, k=10, method="randomized", precision="double", maxit=1)
    refp = reference("hawaiibirds", 10, True, 1)
    assert rp["misc"]["iters_per_factor"].tolist() == [1] and np.allclose(rp["misc"]["row_means"], refp["row_means"])
    assert np.max(np.abs(rp["d"] - refp["d"])) <= 1e-12 * refp["d"][0]
    # method = "auto" at 32 <= k < 64 is unchanged: the reference entry's Lanczos under the name R resolves
    ra = S.pca(A, k=40)
    lz = _abi.svd_pca(parts(A), 40, precision="float", tol=1e-5, max_iter=3, center=True, seed=0, algorithm=3)
    assert lz["status"] == 0, lz["error"]
    assert ra["misc"]["method"] == "randomized" and ra["misc"]["iters_per_factor"][0] == lz["iters"][0] >= 40
    assert np.array_equal(ra["d"], lz["d"][:40]) and np.array_equal(ra["u"], lz["U"][:, :40]) and np.array_equal(ra["v"], lz["V"][:, :40])
