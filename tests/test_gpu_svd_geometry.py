"""The SVD family's block reductions beyond one chunk (rcppml_amd/csrc/kernels_svd.hip.h, kernels_svd_reg.hip.h, kernels_svd_cv.hip.h:
a block sums CH = 2048 elements into P[block * np + c], every consumer re-adds all blocks in order, ops_svd.hip sizes it with
nblk(len)): plain, regularised and cross-validated deflation against the numpy restatement, Lanczos against numpy's dense SVD and
the NMF start against LAPACK, at the shapes of tests/svd_geometry_inputs.py -- two to four blocks a side, a chunk that is exactly
full, last chunks of one element, nbm != nbn, and test_loss over 12 to 411 blocks.  What those inputs promise (spectra, fixed
iteration counts, the restatement's own precision) is proved in tests/test_svd_geometry_cpu.py.

Bounds: the project's own.  fp64 deflation of any kind: equal iters, k, k_computed, n_test and n_masked; u, d, v (each relative to
its largest reference magnitude) and every test loss within 1e-10; row_means at rtol 1e-12; frob within 1e-12 -- what
test_gpu_svd.py, test_gpu_svd_cv.assert_parity and test_gpu_svd_reg.py assert.  fp32: the same counts and a deviation of at most
4 * MEASURED[case], the factor those files use.  Lanczos and the NMF start: the limits of test_lanczos_against_numpy and of
test_gpu_nmf_init.py.

The degenerate shapes (1 x 2049, 2049 x 1; k = 1, centre off): no entry refuses them.  Deflation matches the restatement like any
other shape.  Lanczos gets min(m, n) = 1 step: at 2049 x 1 that step is exact and the result is numpy's; at 1 x 2049 one step from
the start vector p_0 gives sigma = |A p_0|, u = +-1 and v = p_0, not the singular triplet (as test_gpu_nmf_init.py notes of its
1 x 9 input), and that is what the test holds it to, with p_0 drawn here from the same stream."""
import functools

import numpy as np
import pytest

import svd_geometry_inputs as G
import svd_reg_ref as R
from rcppml_amd import _abi
from rcppml_amd.data import splitmix64_uniform
from test_gpu_nmf_init import LIMIT, assert_start_is_the_ritz_path_transformed, lapack_gap, spectrum_matrix, start

pytestmark = pytest.mark.gpu
IDS = dict(ids=G.case_id)
PRECISIONS = ("double", "float")
DT = {"double": np.float64, "float": np.float32}


def csc_of(pattern, values=None):
    """(p, i[, x], rows, cols) of a bool pattern, column by column; stored zeros stay stored."""
    cols, rows = np.nonzero(pattern.T)
    p = np.concatenate([[0], np.cumsum(pattern.sum(axis=0))]).astype(np.int32)
    x = () if values is None else (values[rows, cols].astype(np.float64),)
    return (p, rows.astype(np.int32)) + x + pattern.shape


@functools.lru_cache(maxsize=None)
def source(shape, kind, level):
    """What the entries take for this input: the array, or the CSC parts of its stored pattern."""
    A, keep = G.shape_input(shape, kind, level)
    return A if keep is None else csc_of(keep, A)


@functools.lru_cache(maxsize=None)
def mask_parts(m, n):
    return csc_of(G.obs_mask(m, n))


def run(case, precision):
    """The case through its entry; the keywords of reg_deflation_svd as the entry takes them."""
    A, keep, kw = G.case_kwargs(case)
    kw = dict(kw)
    args = dict(dense=keep is None, precision=precision, max_iter=kw.pop("maxit"))
    if kw.pop("obs_mask", None) is not None:
        args["obs_mask"] = mask_parts(*A.shape)
    lam = kw.pop("graph_lambda", (0, 0))
    for side, l in (("graph_u", lam[0]), ("graph_v", lam[1])):
        if kw.get(side) is not None:
            args[side] = R.graph_csc(kw.pop(side), l)
    args.update(kw)
    src, k = source(case[1], G.case_kind(case), G.case_center(case)), G.case_k(case)
    if case[0] == "defl":
        r = _abi.svd_pca(src, k, algorithm=0, **args)
    else:
        r = (_abi.svd_reg if case[0] == "reg" else _abi.svd_cv)(src, k, **args)
    assert r["status"] == 0, r["error"]
    return r


def as_result(r):
    ks = r["k"]
    return dict(u=r["U"][:, :ks], d=r["d"][:ks], v=r["V"][:, :ks])


def assert_counts(case, r, ref):
    kc = ref["k_computed"]
    assert r["k"] == ref["k_selected"] == G.case_k(case)
    assert np.array_equal(r["iters"][:kc], ref["iters"])
    if case[0] != "defl":                                   # the reference-shaped entry has no such outputs
        assert (r["k_computed"], r["n_test"], r["n_masked"]) == (kc, ref["n_test"], ref["n_masked"])


# ------------------------------------------------------------------------------------------------ deflation, reg, cv
@pytest.mark.parametrize("case", G.PARITY_CASES, **IDS)
def test_fp64_parity(case):
    ref = G.case_ref(case)
    r = run(case, "double")
    assert_counts(case, r, ref)
    dev = R.deviation(as_result(r), ref)
    print("%s double: deviation %.3e bound 1e-10" % (G.case_id(case), dev))
    assert dev <= 1e-10
    tl, kc = ref["test_loss"], ref["k_computed"]
    if tl.size:
        print("%s double: test loss deviation %.3e over %d entries" % (G.case_id(case), np.max(np.abs(r["test_loss"][:kc] - tl) / tl), ref["n_test"]))
        assert np.all(np.abs(r["test_loss"][:kc] - tl) <= 1e-10 * tl)
    if ref["row_means"] is not None:
        assert np.allclose(r["row_means"], ref["row_means"], rtol=1e-12, atol=0)
    assert abs(r["frob"] - ref["frob"]) <= 1e-12 * abs(ref["frob"])


@pytest.mark.parametrize("case", G.PARITY_CASES, **IDS)
def test_fp32_parity(case):
    ref = G.case_ref(case)
    r = run(case, "float")
    assert_counts(case, r, ref)
    dev, bound = R.deviation(as_result(r), ref), 4 * G.MEASURED[case]
    print("%s float: deviation %.3e bound %.3e share %.2f" % (G.case_id(case), dev, bound, dev / bound))
    assert dev <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", G.DETERMINISM_CASES, **IDS)
def test_two_runs_are_bitwise_identical(case, precision):
    a, b = run(case, precision), run(case, precision)
    for key in ("U", "V", "d", "iters", "test_loss"):
        assert np.array_equal(a[key], b[key]), key
    assert a["k"] == b["k"] == G.case_k(case)


# ------------------------------------------------------------------------------------------------ Lanczos
def one_step_lanczos(D, seed, dt):
    """What one Lanczos step from p_0 = normalise(uniform - 0.5) leaves of a one-row matrix: sigma = |D p_0|, u = +-1, v = p_0."""
    p0 = splitmix64_uniform(42 if seed == 0 else seed, 0, D.shape[1], dt).astype(np.float64) - 0.5
    p0 /= np.linalg.norm(p0)
    return np.abs(D @ p0), p0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", G.LANCZOS_CASES, **IDS)
def test_lanczos_against_numpy(case, precision):
    shape, kind, center = case
    D, sv, means = G.lanczos_ref(*case)
    k = G.lanczos_k(shape)
    tol, lim = (1e-12, 1e-8) if precision == "double" else (1e-6, 1e-4)
    r = _abi.svd_pca(source(shape, kind, center), k, dense=kind == "dense", precision=precision, tol=tol, max_iter=300, center=center, seed=0,
                     algorithm=2)
    assert r["status"] == 0, r["error"]
    assert r["k"] == k and r["iters"][0] >= k
    d, U, V = r["d"][:k], r["U"][:, :k], r["V"][:, :k]
    if D.shape[0] == 1:                                       # one step: see the module's docstring
        sv, p0 = one_step_lanczos(D, 0, DT[precision])
        assert r["iters"][0] == 1 and np.max(np.abs(np.abs(V[:, 0]) - np.abs(p0))) < lim
    near = np.min(np.abs(d[:, None] - sv[None, :]) / sv[None, :], axis=1)
    print("%s %s: steps %d, nearest %.3e, ordered %.3e" % (G.case_id(case), precision, r["iters"][0], np.max(near),
                                                           np.max(np.abs(d - sv[:k]) / sv[:k])))
    assert np.max(near) < lim
    assert np.max(np.abs(d - sv[:k]) / sv[:k]) < 1e-4
    assert np.max(np.abs(U.T @ U - np.eye(k))) < lim and np.max(np.abs(V.T @ V - np.eye(k))) < lim
    if center:
        assert np.allclose(r["row_means"], means, rtol=1e-12, atol=1e-300)
    assert abs(r["frob"] - np.sum(D * D)) <= 1e-10 * np.sum(D * D)


# ------------------------------------------------------------------------------------------------ NMF start
@functools.lru_cache(maxsize=None)
def nmf_matrix(key):
    """(A, its LAPACK SVD): spectrum_matrix of test_gpu_nmf_init.py, the second the transpose of the first as there."""
    A = spectrum_matrix(513, 257)
    if key == "257x513":
        A = np.ascontiguousarray(A.T)
    assert A.shape == G.NMF_SHAPES[key]
    return A, np.linalg.svd(A, full_matrices=False)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", G.NMF_CASES, **IDS)
def test_nmf_start_against_lapack(case, precision):
    key, k, kind = case
    A, usv = nmf_matrix(key)
    r = start(A, k, kind == "dense", precision)
    assert r["k_svd"] == k and 0 < r["iters"] <= max(3 * k, k + 50)
    gap, dgap = lapack_gap(r, usv, k), np.max(np.abs(r["d"] - usv[1][:k])) / usv[1][0]
    print("%s %s: steps %d, factor gap %.3e, sigma gap %.3e" % (G.case_id(case), precision, r["iters"], gap, dgap))
    assert gap < LIMIT[precision] and dgap < LIMIT[precision]
    assert np.all(r["W_T"] >= 0) and np.all(r["H"] >= 0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", G.NMF_CASES, **IDS)
def test_nmf_start_is_bitwise_the_ritz_path_transformed(case, precision):
    key, k, kind = case
    assert_start_is_the_ritz_path_transformed(nmf_matrix(key)[0], k, kind == "dense", precision)
