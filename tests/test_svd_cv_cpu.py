"""CPU checks of the cross-validated / auto-rank / masked SVD: the numpy restatement (tests/svd_cv_ref.py, the GPU path's parity
target) against the pinned reference hash vectors and against svd_ref, the conditions the GPU parity inputs must meet, R's
validation messages and resolution rules, and the entries' refusals that hold before any device work.  No GPU needed."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import svd_cv_ref as C
import svd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hash_and_holdout_reproduce_the_pinned_reference_vectors():
    z = np.load(os.path.join(HERE, "golden", "ref_vectors.npz"))
    ii, jj = z["hash_i"], z["hash_j"]
    for seed in (42, 7):
        assert np.array_equal(C.cv_hash(seed, ii, jj), z["hash_seed%d" % seed].astype(np.uint64)), seed
        assert np.array_equal(C.is_holdout(seed, ii, jj, 10), z["holdout_seed%d_inv10" % seed].astype(bool)), seed
        assert 0 < z["holdout_seed%d_inv10" % seed].sum()


def test_effective_seed_rule():
    assert C.effective_cv_seed(0, 0) == 42
    assert C.effective_cv_seed(7, 0) == 7 ^ 0xBEEF
    assert C.effective_cv_seed(7, 9) == 9


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("cons", [dict(), dict(nonneg=(True, True)), dict(L1=(0.02, 0.02))])
def test_without_cv_the_restatement_is_svd_ref(center, cons):
    A = C.dense_input()
    a = C.cv_deflation_svd(A, 5, center=center, **cons)
    b = R.deflation_svd(A, 5, center=center, **cons)
    for key in ("u", "d", "v", "iters"):
        assert np.array_equal(a[key], b[key]), key
    assert a["frob"] == b["frob"] and a["k_selected"] == a["k_computed"] == len(b["d"])
    assert a["test_loss"].size == 0 and a["n_test"] == 0


def parity_cases():
    S, keep = C.sparse_input()
    out = []
    for center in (False, True):
        out.append(("dense", center, False, C.dense_input(), None))
        for mz in (False, True):
            out.append(("sparse", center, mz, S, keep))
    return out


@pytest.mark.parametrize("case", parity_cases(), ids=lambda c: "%s-center%d-mz%d" % (c[0], c[1], c[2]))
def test_parity_inputs_meet_their_conditions(case):
    """What keeps the GPU's patience decisions from flipping on summation order: an interior minimum, a stop by patience, and
    consecutive test losses at least 1e-3 apart (relative)."""
    _, center, mz, A, keep = case
    r = C.cv_deflation_svd(A, C.K_MAX, stored=keep, center=center, mask_zeros=mz, **C.CV_KW)
    tl = r["test_loss"]
    assert 1 < r["k_selected"] < r["k_computed"] <= C.K_MAX
    assert r["stopped_by_patience"] and r["k_computed"] == r["k_selected"] + C.CV_KW["patience"]
    assert int(np.argmin(tl)) + 1 == r["k_selected"]
    steps = np.abs(np.diff(tl)) / np.minimum(tl[1:], tl[:-1])
    assert steps.min() >= 1e-3, steps
    assert r["n_test"] > 0 and len(r["d"]) == r["k_selected"]
    if keep is not None:
        assert np.all(keep[r["rows"], r["cols"]])            # sparse: stored entries only, with either mask_zeros


def test_test_entries_are_column_major_and_training_excludes_them():
    S, keep = C.sparse_input()
    r = C.cv_deflation_svd(S, 2, stored=keep, **C.CV_KW)
    lin = r["cols"].astype(np.int64) * S.shape[0] + r["rows"]
    assert np.all(np.diff(lin) > 0)
    frac = r["n_test"] / keep.sum()
    assert 0.07 < frac < 0.13


def test_fixed_k_may_return_fewer_factors_and_tiny_fraction_gives_rank_one():
    A = C.dense_input()
    r = C.cv_deflation_svd(A, 10, test_fraction=0.1)
    assert r["k_selected"] < r["k_computed"] < 10
    z = C.cv_deflation_svd(A, C.K_MAX, test_fraction=1e-9)
    assert z["n_test"] == 0 and np.all(z["test_loss"] == 0)
    assert z["k_selected"] == 1 and z["k_computed"] == 1 + 3


def test_obs_mask_zeroes_training_values_only():
    S, keep = C.sparse_input()
    rng = np.random.default_rng(5)
    mask = rng.random(S.shape) < 0.05                        # stored and unstored positions
    r = C.cv_deflation_svd(S, 3, stored=keep, obs_mask=mask)
    assert r["n_masked"] == int((mask & keep).sum()) and 0 < r["n_masked"] < mask.sum()
    Z = S.copy()
    Z[mask] = 0
    b = R.deflation_svd(Z, 3)
    assert np.array_equal(r["d"], b["d"]) and np.array_equal(r["u"], b["u"])
    assert r["frob"] == float(np.sum(S * S))                 # the norm is the full matrix's


# ------------------------------------------------------------------------------------------------ surface
def test_cv_resolution_is_rs():
    from rcppml_amd.svd import resolve_cv
    assert resolve_cv("auto") == (50, "deflation", 0.05, True)
    assert resolve_cv("auto", k_max=20, test_fraction=0.2) == (20, "deflation", 0.2, True)
    assert resolve_cv(10, test_fraction=0.1) == (10, "deflation", 0.1, False)
    assert resolve_cv(10, test_fraction=0.1, nonneg=True) == (10, "krylov", 0.1, False)
    assert resolve_cv(5, test_fraction=0.1, nonneg=True) == (5, "deflation", 0.1, False)
    assert resolve_cv(5, "lanczos", test_fraction=0.1) == (5, "lanczos", 0.0, False)        # CV dropped silently
    assert resolve_cv(5, "krylov", test_fraction=0.1) == (5, "krylov", 0.1, False)
    assert resolve_cv(5) == (5, "auto", 0.0, False)


@pytest.mark.parametrize("kw, msg", [
    (dict(k=5, test_fraction=-0.1), "'test_fraction' must be in [0, 1)"),
    (dict(k=5, test_fraction=1), "'test_fraction' must be in [0, 1)"),
    (dict(k="auto", patience=0), "'patience' must be >= 1"),
    (dict(k=0), "'k' must be >= 1"),
    (dict(k="auto", method="lanczos"), "method 'lanczos' does not support auto-rank. Use 'deflation' or 'krylov'."),
    (dict(k="auto", method="randomized"), "method 'randomized' does not support auto-rank. Use 'deflation' or 'krylov'."),
    (dict(k="auto", method="qr"), "method must be one of: auto, deflation, krylov, lanczos, irlba, randomized"),
])
def test_cv_validation_messages_are_rs(kw, msg):
    from rcppml_amd.svd import resolve_cv
    kw = dict(kw)
    with pytest.raises(ValueError) as e:
        resolve_cv(kw.pop("k"), **kw)
    assert str(e.value) == msg


def test_mask_forms_and_messages_are_rs():
    from rcppml_amd.svd import resolve_mask
    Mk = sp.csc_matrix(np.array([[0, 1.0], [2.0, 0], [0, 3.0]]))
    assert resolve_mask(None, (3, 2)) == (False, None)
    assert resolve_mask("zeros", (3, 2)) == (True, None)
    mz, (p, i, rows, cols) = resolve_mask(Mk, (3, 2))
    assert not mz and list(p) == [0, 1, 3] and list(i) == [1, 0, 2] and (rows, cols) == (3, 2)
    mz, obs = resolve_mask(("zeros", Mk), (3, 2))
    assert mz and list(obs[1]) == [1, 0, 2]
    for bad, msg in ((("ones", Mk), "'mask' list must be list(\"zeros\", <matrix>)"),
                     (("zeros",), "'mask' list must be list(\"zeros\", <matrix>)"),
                     ("nonzeros", "'mask' string must be \"zeros\". Got: 'nonzeros'"),
                     (np.ones((3, 2)), "'mask' must be NULL, 'zeros', a dgCMatrix, or list(\"zeros\", <dgCMatrix>)"),
                     (sp.csc_matrix((2, 2)), "'mask' dimensions (2 x 2) must match 'A' (3 x 2)")):
        with pytest.raises(ValueError) as e:
            resolve_mask(bad, (3, 2))
        assert str(e.value) == msg


def test_surface_raises_rs_messages_before_any_device_work():
    from rcppml_amd import svd as S
    A = C.dense_input()
    with pytest.raises(ValueError) as e:
        S.svd(A, k="auto", method="lanczos")
    assert str(e.value) == "method 'lanczos' does not support auto-rank. Use 'deflation' or 'krylov'."
    with pytest.raises(ValueError) as e:
        S.pca(A, k=3, test_fraction=1.5)
    assert str(e.value) == "'test_fraction' must be in [0, 1)"
    with pytest.raises(ValueError) as e:
        S.svd(A, k=3, mask="nonzero")
    assert str(e.value) == "'mask' string must be \"zeros\". Got: 'nonzero'"


# ------------------------------------------------------------------------------------------------ entries
def test_header_declares_the_cv_entries_and_library_exports_them():
    import re
    from rcppml_amd import _abi
    src = open(os.path.join(os.path.dirname(HERE), "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_svd_cv_ex", 42), ("rcppml_gpu_svd_cv_dense_ex", 39)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert m.group(1).count("*") == count and len(m.group(1).split(",")) == count, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name), name


def _csc(A):
    S = sp.csc_matrix(A)
    S.sort_indices()
    return (S.indptr, S.indices, S.data, A.shape[0], A.shape[1])


GOOD_MASK = ([0] * 41, [], 60, 40)


@pytest.mark.parametrize("kw, word", [
    (dict(patience=0), "patience"),
    (dict(test_fraction=1.0), "test_fraction"),
    (dict(test_fraction=-0.5), "test_fraction"),
    (dict(k=0), "k_max"),
    (dict(k=41), "k_max"),
    (dict(max_iter=0), "max_iter"),
    (dict(obs_mask=([0] * 61, [], 40, 60)), "obs_mask dimensions"),
    (dict(obs_mask=([1] + [1] * 40, [0], 60, 40)), "malformed CSC"),
    (dict(obs_mask=([0, 2] + [2] * 39, [3, 1], 60, 40)), "malformed CSC"),              # rows not increasing
    (dict(obs_mask=([0, 1] + [1] * 39, [60], 60, 40)), "malformed CSC"),                # row out of range
])
def test_cv_entry_refusals_leave_buffers_untouched(kw, word):
    """Refused before any device work, so these hold with or without a GPU."""
    from rcppml_amd import _abi
    A = C.dense_input()
    kw = dict(kw)
    k = kw.pop("k", 3)
    kb = max(k, 1)
    for dense, prec in ((False, "double"), (True, "float")):
        bufs = dict(U=np.full(60 * kb, 7.0), d=np.full(kb, 7.0), V=np.full(40 * kb, 7.0), row_means=np.full(60, 7.0),
                    iters=np.full(kb, 7, np.int32), test_loss=np.full(kb, 7.0))
        args = dict(dict(test_fraction=0.1, center=True), **kw)
        r = _abi.svd_cv(A if dense else _csc(A), k, dense=dense, precision=prec, buffers=bufs, **args)
        assert r["status"] == -1 and word in r["error"], r["error"]
        assert all(np.all(b == 7) for b in bufs.values())
        assert (r["k"], r["k_computed"], r["n_test"], r["n_masked"], r["frob"], r["wall_ms"]) == (0, 0, 0, 0, 0.0, 0.0)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    from rcppml_amd import _abi, svd
    with pytest.raises(_abi.BackendError):
        svd.pca(C.dense_input(), k="auto")
