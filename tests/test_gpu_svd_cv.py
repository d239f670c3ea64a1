"""GPU cross-validated / auto-rank / masked deflation SVD (rcppml_gpu_svd_cv_ex, rcppml_gpu_svd_cv_dense_ex: rcppml_amd/csrc/ops_svd.hip,
kernels_svd_cv.hip.h) against the numpy restatement of the reference's CPU path (tests/svd_cv_ref.py), against the plain
deflation entries bit for bit where the two must coincide, and through the Python surface."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_cv_ref as C
from rcppml_amd import _abi, svd as S

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K = C.K_MAX
# (vi) The restatement run with dtype = np.float32 deviates from its float64 run by at most 3.9e-7 (relative, over the six planted
# cases: dense / sparse, centred or not, both mask_zeros); the fp32 device trajectory may deviate four times that from the float64
# restatement -- kernel and numpy summation orders differ and the deviation compounds over up to 12 factors.
F32_TRAJECTORY_MEASURED = 3.9e-7
F32_TRAJECTORY_BOUND = 4 * F32_TRAJECTORY_MEASURED


def parts_of(A, keep, x=None):
    """CSC parts of the stored pattern `keep` (explicit zeros stay stored)."""
    cols, rows = np.nonzero(keep.T)
    p = np.concatenate([[0], np.cumsum(keep.sum(axis=0))]).astype(np.int32)
    return (p, rows.astype(np.int32), (A if x is None else x)[rows, cols].astype(np.float64), A.shape[0], A.shape[1])


def mask_of(mask):
    cols, rows = np.nonzero(mask.T)
    p = np.concatenate([[0], np.cumsum(mask.sum(axis=0))]).astype(np.int32)
    return (p, rows.astype(np.int32), mask.shape[0], mask.shape[1])


@functools.lru_cache(maxsize=None)
def inputs():
    Sp, keep = C.sparse_input()
    return dict(dense=(C.dense_input(), None), sparse=(Sp, keep))


def run_gpu(A, keep, k=K, precision="double", obs_mask=None, **kw):
    src = A if keep is None else parts_of(A, keep)
    r = _abi.svd_cv(src, k, dense=keep is None, precision=precision, obs_mask=None if obs_mask is None else mask_of(obs_mask), **kw)
    assert r["status"] == 0, r["error"]
    return r


def run_ref(A, keep, k=K, dtype=np.float64, **kw):
    kw = dict(kw)
    kw["maxit"] = kw.pop("max_iter", 200)
    if "upper_bound" in kw:
        kw["ub"] = kw.pop("upper_bound")
    return C.cv_deflation_svd(A, k, stored=keep, dtype=dtype, **kw)


def assert_parity(r, ref, center=False):
    ks, kc = ref["k_selected"], ref["k_computed"]
    assert (r["k"], r["k_computed"], r["n_test"], r["n_masked"]) == (ks, kc, ref["n_test"], ref["n_masked"])
    assert np.array_equal(r["iters"][:kc], ref["iters"])
    for a, b in ((r["U"][:, :ks], ref["u"]), (r["d"][:ks], ref["d"]), (r["V"][:, :ks], ref["v"])):
        assert np.max(np.abs(a - b)) <= 1e-10 * max(np.max(np.abs(b)), 1e-300)
    tl = ref["test_loss"]
    if tl.size:
        print("test_loss rel dev", np.max(np.abs(r["test_loss"][:kc] - tl) / np.maximum(tl, 1e-300)) if np.all(tl > 0) else 0.0)
        assert np.all(np.abs(r["test_loss"][:kc] - tl) <= 1e-10 * tl)
    if center:
        assert np.allclose(r["row_means"], ref["row_means"], rtol=1e-12, atol=0)
    assert abs(r["frob"] - ref["frob"]) <= 1e-12 * abs(ref["frob"])


PLANTED = [("dense", False), ("sparse", False), ("sparse", True)]
CONS = [dict(), dict(nonneg=(True, True))]


# ------------------------------------------------------------------------------------------------ (i) fp64 parity
@pytest.mark.parametrize("name, mask_zeros", PLANTED)
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("ci", range(len(CONS)))
def test_fp64_parity_on_the_planted_inputs(name, mask_zeros, center, ci):
    A, keep = inputs()[name]
    kw = dict(test_fraction=0.1, patience=3, tol=1e-5, max_iter=200, center=center, mask_zeros=mask_zeros, **CONS[ci])
    assert_parity(run_gpu(A, keep, **kw), run_ref(A, keep, **kw), center)


# ------------------------------------------------------------------------------------------------ (ii) shapes
def odd_input():
    """65 x 63 at density 0.3: not a multiple of the wavefront or of the elementwise chunk."""
    A = C.planted(65, 63, (40.0, 25, 12), 11)
    keep = np.random.default_rng(12).random(A.shape) < 0.3
    return A * keep, keep


def test_odd_shape():
    A, keep = odd_input()
    for center in (False, True):
        kw = dict(test_fraction=0.1, center=center, max_iter=200)
        assert_parity(run_gpu(A, keep, **kw), run_ref(A, keep, **kw), center)
        assert_parity(run_gpu(A, None, **kw), run_ref(A, None, **kw), center)      # the same matrix through the dense entry


def test_empty_row_and_column():
    A, keep = odd_input()
    keep = keep.copy()
    keep[7, :] = False
    keep[:, 3] = False
    A = A * keep
    kw = dict(test_fraction=0.1, center=True, mask_zeros=True)
    assert_parity(run_gpu(A, keep, **kw), run_ref(A, keep, **kw), True)


def test_a_column_held_out_entirely():
    A, keep = odd_input()
    keep = keep.copy()
    keep[:, 5] = False
    keep[[9, 40], 5] = True                                   # two stored entries; look for a mask seed that holds both out
    A = C.planted(65, 63, (40.0, 25, 12), 11) * keep
    thr = np.uint64(C.M64 // 10)
    seed = next(s for s in range(1, 100000) if np.all(C.cv_hash(s, np.array([9, 40]), np.array([5, 5])) < thr))
    kw = dict(test_fraction=0.1, cv_seed=seed)
    ref = run_ref(A, keep, **kw)
    assert np.sum(ref["cols"] == 5) == 2
    assert_parity(run_gpu(A, keep, **kw), ref)


def test_no_test_entries_gives_rank_one_after_patience():
    A, keep = inputs()["sparse"]
    for kp in (keep, None):
        r = run_gpu(A, kp, test_fraction=1e-9, patience=3)
        assert r["n_test"] == 0 and (r["k"], r["k_computed"]) == (1, 4)
        assert np.all(r["test_loss"][:4] == 0)
        assert_parity(r, run_ref(A, kp, test_fraction=1e-9, patience=3))


# ------------------------------------------------------------------------------------------------ (iii) obs_mask
def the_mask(shape):
    return np.random.default_rng(21).random(shape) < 0.06     # stored and unstored positions


@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("tf", [0.0, 0.1])
def test_obs_mask_parity(name, tf):
    A, keep = inputs()[name]
    mask = the_mask(A.shape)
    if keep is not None:
        assert np.any(mask & keep) and np.any(mask & ~keep)
    kw = dict(test_fraction=tf, center=True, max_iter=200)
    k = K if tf > 0 else 4
    r = run_gpu(A, keep, k=k, obs_mask=mask, **kw)
    ref = run_ref(A, keep, k=k, obs_mask=mask, **kw)
    assert r["n_masked"] == ref["n_masked"] == int((mask & (keep if keep is not None else True)).sum())
    assert_parity(r, ref, True)


def test_obs_mask_without_cv_is_the_plain_entry_on_stored_zeros():
    A, keep = inputs()["sparse"]
    mask = the_mask(A.shape)
    r = run_gpu(A, keep, k=4, obs_mask=mask)
    Z = np.where(mask, 0.0, A)
    b = _abi.svd_pca(parts_of(A, keep, x=Z), 4, precision="double", algorithm=0)
    assert b["status"] == 0, b["error"]
    assert r["k"] == b["k"] == 4
    for key in ("U", "d", "V", "iters"):
        assert np.array_equal(r[key], b[key]), key


# ------------------------------------------------------------------------------------------------ (iv) plain call
@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("center", [False, True])
def test_plain_call_is_the_existing_deflation_bit_for_bit(name, precision, center):
    A, keep = inputs()[name]
    kw = dict(precision=precision, center=center, nonneg=(True, False), L1=(0.0, 0.01))
    r = run_gpu(A, keep, k=5, **kw)
    b = _abi.svd_pca(A if keep is None else parts_of(A, keep), 5, dense=keep is None, algorithm=0, **kw)
    assert b["status"] == 0, b["error"]
    assert r["k"] == r["k_computed"] == b["k"] and r["n_test"] == 0
    for key in ("U", "d", "V", "iters", "row_means"):
        assert np.array_equal(r[key], b[key]), key
    assert r["frob"] == b["frob"]


# ------------------------------------------------------------------------------------------------ (v) repeatability
@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("precision", ["double", "float"])
def test_two_runs_are_bitwise_identical(name, precision):
    A, keep = inputs()[name]
    kw = dict(precision=precision, test_fraction=0.1, center=True, obs_mask=the_mask(A.shape))
    a, b = run_gpu(A, keep, **kw), run_gpu(A, keep, **kw)
    assert a["k"] == b["k"] and a["k_computed"] == b["k_computed"]
    for key in ("U", "d", "V", "test_loss", "iters"):
        assert np.array_equal(a[key], b[key]), key


# ------------------------------------------------------------------------------------------------ (vi) fp32
@pytest.mark.parametrize("name, mask_zeros", PLANTED)
@pytest.mark.parametrize("center", [False, True])
def test_fp32_against_the_fp64_restatement(name, mask_zeros, center):
    A, keep = inputs()[name]
    kw = dict(test_fraction=0.1, patience=3, tol=1e-5, max_iter=200, center=center, mask_zeros=mask_zeros)
    ref = run_ref(A, keep, **kw)
    r64 = run_gpu(A, keep, **kw)
    r = run_gpu(A, keep, precision="float", **kw)
    assert r["k"] == r64["k"] == ref["k_selected"]
    ks, kc = r["k"], min(r["k_computed"], ref["k_computed"])
    assert np.max(np.abs(r["d"][:ks] - ref["d"])) <= 1e-4 * ref["d"][0]
    dev = np.max(np.abs(r["test_loss"][:kc] - ref["test_loss"][:kc]) / ref["test_loss"][:kc])
    print("fp32 trajectory deviation", dev, "bound", F32_TRAJECTORY_BOUND)
    assert r["k_computed"] == ref["k_computed"]
    assert dev <= F32_TRAJECTORY_BOUND


# ------------------------------------------------------------------------------------------------ (vii) surface
def hawaiibirds():
    z = np.load(os.path.join(HERE, "golden", "hawaiibirds.npz"))
    A = sp.csc_matrix((z["x"].astype(np.float64), z["i"], z["p"]), shape=tuple(int(v) for v in z["shape"]))
    A.sort_indices()
    return A


def test_python_surface():
    A = hawaiibirds()
    r = S.svd(A, k="auto", precision="double")
    mi = r["misc"]
    assert len(r["d"]) == mi["k_selected"] <= 50 and mi["auto_rank"] is True and mi["method"] == "deflation"
    assert len(mi["test_loss"]) == len(mi["iters_per_factor"]) >= mi["k_selected"] and mi["n_test"] > 0
    assert r["u"].shape == (183, mi["k_selected"]) and r["v"].shape == (1183, mi["k_selected"])
    assert mi["cv_seed_effective"] == 42
    r = S.pca(A, k=6, test_fraction=0.1, mask="zeros")
    assert 1 <= len(r["d"]) <= 6 and r["misc"]["auto_rank"] is False
    assert np.allclose(r["misc"]["row_means"], A.toarray().mean(axis=1), rtol=1e-12, atol=1e-300)
    with pytest.raises(ValueError) as e:
        S.svd(A, k="auto", method="lanczos")
    assert str(e.value) == "method 'lanczos' does not support auto-rank. Use 'deflation' or 'krylov'."
    with pytest.raises(_abi.BackendError):
        S.svd(A, k=10, nonneg=True, test_fraction=0.1)       # R resolves this to krylov, which the GPU refuses
    m = sp.random(183, 1183, density=0.01, format="csc", random_state=3)
    r = S.svd(A, k=3, method="deflation", mask=m, precision="double")
    assert len(r["d"]) == 3 and r["misc"]["n_test"] == 0 and r["misc"]["test_loss"].size == 0
