"""CPU-only checks of label-guided refinement: hand-worked answers of the numpy restatement (tests/refine_ref.py), the properties the
reference's own tests assert (test_compute_target.R, test_refine.R) on the restatement, R's validation messages on the public
functions, and the ABI's refusals (decided on the host, nothing written) and its no-device behaviour."""
import os

import numpy as np
import pytest

import refine_ref as R
from rcppml_amd import _abi
from rcppml_amd import compute_target, refine
from rcppml_amd.nmf import NMFModel
from rcppml_amd.refine import as_factor

NO_GPU = not os.path.exists("/dev/kfd")


def emb(k, n, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (k, n))


# ------------------------------------------------------------------------------------------------ the restatement, by hand
def test_two_classes_unwhitened_by_hand():
    H = emb(2, 10, 1)
    codes = np.array([0, 1] * 5)
    T = R.compute_target(H, codes, 2, whiten=False)
    c0, c1 = H[:, codes == 0].mean(axis=1), H[:, codes == 1].mean(axis=1)
    gm = (c0 + c1) / 2
    assert np.allclose(T[:, codes == 0], (c0 - gm)[:, None], rtol=0, atol=1e-15)
    assert np.allclose(T[:, codes == 1], (c1 - gm)[:, None], rtol=0, atol=1e-15)
    assert np.abs(T.sum(axis=1)).max() < 1e-14                  # balanced classes: the rows sum to 0


def test_single_class_gives_exactly_zero():
    H = emb(3, 9, 2)
    for whiten in (False, True):
        assert np.array_equal(R.compute_target(H, np.zeros(9, int), 1, whiten=whiten), np.zeros((3, 9)))


def test_na_columns_are_exactly_zero():
    H = emb(3, 12, 3)
    codes = np.array([0, 1, 2, -1] * 3)
    for whiten in (False, True):
        T = R.compute_target(H, codes, 3, whiten=whiten)
        assert np.array_equal(T[:, codes < 0], np.zeros((3, 3)))
        assert np.abs(T[:, codes >= 0]).min() > 0


def test_zca_whitens_the_shrunk_covariance():
    H = emb(4, 60, 4)
    codes = np.arange(60) % 6
    det = {}
    R.compute_target(H, codes, 6, whiten=True, detail=det)
    assert not det["floored"].any()
    W = det["W_zca"]
    assert np.abs(W @ det["S_shrunk"] @ W - np.eye(4)).max() < 1e-10


def test_empty_class_keeps_a_zero_centroid_and_stays_out_of_the_grand_mean():
    H = emb(2, 8, 5)
    codes = np.array([0, 2] * 4)                                 # class 1 of 3 is empty
    T = R.compute_target(H, codes, 3, whiten=False)
    c0, c2 = H[:, codes == 0].mean(axis=1), H[:, codes == 2].mean(axis=1)
    assert np.allclose(T[:, 0], c0 - (c0 + c2) / 2, rtol=0, atol=1e-15)


def test_variant_of_the_restatement_agrees_to_rounding():
    H = emb(5, 200, 6)
    codes = np.random.default_rng(7).integers(0, 4, 200)
    a = R.compute_target(H, codes, 4, True)
    b = R.compute_target(H, codes, 4, True, variant=True)
    assert 0 < R.rel_diff(a, b) < 1e-10 or np.array_equal(a, b)


# ------------------------------------------------------------------------------- the reference's own properties (restatement)
def test_dimensions_and_balanced_row_means():
    H = emb(4, 30, 8)
    codes = np.arange(30) % 3
    for whiten in (False, True):
        assert R.compute_target(H, codes, 3, whiten=whiten).shape == (4, 30)
    assert np.abs(R.compute_target(H, codes, 3, whiten=False).mean(axis=1)).max() < 1e-10


def test_lambda_zero_returns_H_and_nonneg_clips():
    H = emb(4, 30, 9)
    codes = np.arange(30) % 3
    assert np.abs(R.stage1(H, codes, 3, 0.0) - H).max() < 1e-10
    assert (R.stage1(H, codes, 3, 1.0, nonneg=True) >= 0).all()
    assert (R.stage1(H, codes, 3, 1.0, nonneg=False) < 0).any()


def test_integer_and_string_labels_agree():
    ints = [3, 1, 2, 1, 3, 2, 1, 1]
    strs = ["c", "a", "b", "a", "c", "b", "a", "a"]
    ci, li = as_factor(ints)
    cs, ls = as_factor(strs)
    assert li == [1, 2, 3] and ls == ["a", "b", "c"]
    assert np.array_equal(ci, cs) and ci.dtype == np.int32
    H = emb(3, 8, 10)
    assert np.array_equal(R.compute_target(H, ci, 3), R.compute_target(H, cs, 3))


def test_missing_labels_are_na():
    codes, levels = as_factor(["x", None, "y", "x"])
    assert levels == ["x", "y"] and codes.tolist() == [0, -1, 1, 0]
    codes, levels = as_factor(np.array([2.0, np.nan, 1.0]))
    assert levels == [1.0, 2.0] and codes.tolist() == [1, -1, 0]
    codes, levels = as_factor(np.ma.masked_array([5, 6, 5], mask=[False, True, False]))
    assert levels == [5] and codes.tolist() == [0, -1, 0]


def test_refine_restatement_cycles_zero_leaves_the_model():
    rng = np.random.default_rng(11)
    W, d, H, A = rng.uniform(size=(20, 3)), rng.uniform(0.5, 2, 3), emb(3, 15, 12), rng.uniform(size=(20, 15))
    codes = np.arange(15) % 2
    W1, d1, H1, Hc = R.refine(W, d, H, A, codes, 2, cycles=0)
    assert np.array_equal(W1, W) and np.array_equal(d1, d) and np.array_equal(H1, H)
    assert np.array_equal(Hc, R.stage1(H, codes, 2, 0.8))
    W2, d2, H2, Hc2 = R.refine(W, d, H, A, codes, 2, cycles=2)
    assert W2.shape == W.shape and (H2 >= 0).all() and (d2 > 0).all() and np.allclose(np.sqrt((H2 ** 2).sum(axis=1)), 1.0)


# --------------------------------------------------------------------------------------------------- R's validation messages
def test_validation_messages():
    H = emb(3, 10, 13)
    lab = np.arange(10) % 2
    with pytest.raises(ValueError, match="'H' must be a k x n matrix"):
        compute_target(np.arange(5.0), [0] * 5)
    with pytest.raises(ValueError, match=r"length\(labels\) must equal ncol\(H\)$"):
        compute_target(H, lab[:9])
    with pytest.raises(ValueError, match=r"length\(labels\) must equal ncol\(H\) \[= 10\]"):
        refine(H, labels=lab[:9])
    with pytest.raises(ValueError, match=r"'lambda' must be in \[0, 1\]"):
        refine(H, labels=lab, lambda_=1.5)
    with pytest.raises(ValueError, match=r"'lambda' must be in \[0, 1\]"):
        refine(H, labels=lab, lambda_=-0.1)
    with pytest.raises(ValueError, match="'data' is required when cycles > 0"):
        refine(H, labels=lab, cycles=1)
    with pytest.raises(ValueError, match="'x' must be an nmf object or a k x n matrix"):
        refine([1, 2, 3], labels=lab)
    with pytest.raises(ValueError, match=r"length\(batch\) must equal ncol\(H\) \[= 10\]"):
        refine(H, labels=lab, batch=lab[:3])


# ------------------------------------------------------------------------------------------------------------------------ ABI
def sentinel_untouched(r):
    for b in r["buffers"]:
        assert np.all(np.asarray(b) == -7)


def inputs(m=12, n=10, k=3, seed=14):
    rng = np.random.default_rng(seed)
    A = rng.uniform(size=(m, n))
    return dict(A=A, W=rng.uniform(size=(m, k)), d=rng.uniform(0.5, 2, k), H=rng.uniform(size=(n, k)), lab=np.arange(n) % 2, m=m, n=n, k=k)


def csc_of(A):
    import scipy.sparse as sp
    S = sp.csc_matrix(A)
    return S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data.astype(np.float64)


def test_compute_target_refusals_write_nothing():
    q = inputs()
    cases = [
        (dict(H=None, k=3, n=10), "null H"),
        (dict(labels=None), "null labels"),
        (dict(k=0), "k must be >= 1"),
        (dict(n=0), "n must be >= 1"),
        (dict(n_classes=-1), "n_classes must be >= 0"),
        (dict(labels=np.array([0, 1, 2] + [0] * 7)), "a label is >= n_classes"),
        (dict(H=np.where(np.arange(30).reshape(10, 3) == 4, np.nan, q["H"])), "H holds a non-finite value"),
    ]
    seen = set()
    for change, msg in cases:
        a = dict(H=q["H"], labels=q["lab"], n_classes=2)
        a.update(change)
        r = _abi.compute_target_double(a.pop("H"), a.pop("labels"), a.pop("n_classes"), True, **a)
        assert r["status"] == -1 and msg in r["error"], (change, r["error"])
        sentinel_untouched(r)
        seen.add(r["error"])
    assert len(seen) == len(cases)                               # every refusal has its own message


def test_refine_refusals_write_nothing():
    q = inputs()
    p, i, x = csc_of(q["A"])
    bad_p = p.copy(); bad_p[3] = bad_p[2] - 1
    bad_i = i.copy(); bad_i[1] = bad_i[0]
    base = dict(csc=(p, i, x), dense=None, W_T=q["W"], d=q["d"], H=q["H"], labels=q["lab"], n_classes=2, lambda_=0.8, cycles=1)
    cases = [
        (dict(dense=q["A"]), "not both"),
        (dict(csc=None), "give the matrix as a CSC or as a dense array"),
        (dict(csc=(bad_p, i, x)), "malformed CSC: col_ptr decreases"),
        (dict(csc=(p, bad_i, x)), "malformed CSC: row indices not strictly increasing"),
        (dict(labels=np.full(q["n"], 2)), "a label is >= n_classes"),
        (dict(lambda_=1.5), "lambda must be in [0, 1]"),
        (dict(lambda_=float("nan")), "lambda must be in [0, 1]"),
        (dict(cycles=-1), "cycles must be >= 0"),
        (dict(W_T=None), "null model array"),
        (dict(labels=None), "null labels"),
        (dict(H=np.where(np.arange(30).reshape(10, 3) == 7, np.inf, q["H"])), "H holds a non-finite value"),
        (dict(W_T=np.where(np.arange(36).reshape(12, 3) == 7, np.nan, q["W"])), "W holds a non-finite value"),
        (dict(d=np.array([1.0, np.nan, 1.0])), "d holds a non-finite value"),
    ]
    for change, msg in cases:
        a = dict(base); a.update(change)
        r = _abi.refine_double(a["csc"], a["dense"], q["m"], q["n"], q["k"], a["W_T"], a["d"], a["H"], a["labels"], a["n_classes"],
                               a["lambda_"], a["cycles"])
        assert r["status"] == -1 and msg in r["error"], (change, r["error"])
        sentinel_untouched(r)
    for dims, msg in (((0, 10, 3), "m must be >= 1"), ((12, 0, 3), "n must be >= 1"), ((12, 10, 0), "k must be >= 1")):
        r = _abi.refine_double((p, i, x), None, *dims, q["W"], q["d"], q["H"], q["lab"], 2, 0.8, 1)
        assert r["status"] == -1 and msg in r["error"], r["error"]
        sentinel_untouched(r)
    r = _abi.refine_double(None, q["A"], q["m"], q["n"], 65, np.ones((q["m"], 65)), np.ones(65), np.ones((q["n"], 65)), q["lab"], 2, 0.8, 1)
    assert r["status"] == -1 and "k <= 64" in r["error"]
    sentinel_untouched(r)


def test_wfit_and_correct_refusals_write_nothing():
    q = inputs()
    r = _abi.refine_wfit_double(None, None, q["m"], q["n"], q["k"], q["d"], q["H"])
    assert r["status"] == -1 and "give the matrix as a CSC or as a dense array" in r["error"]
    sentinel_untouched(r)
    r = _abi.refine_wfit_double(None, q["A"], q["m"], q["n"], q["k"], None, q["H"])
    assert r["status"] == -1 and "null d" in r["error"]
    sentinel_untouched(r)
    r = _abi.refine_correct_double(q["H"], q["lab"], 2, -0.5)
    assert r["status"] == -1 and "lambda must be in [0, 1]" in r["error"]
    sentinel_untouched(r)
    r = _abi.refine_correct_double(q["H"], q["lab"] + 1, 2, 0.5)
    assert r["status"] == -1 and "a label is >= n_classes" in r["error"]
    sentinel_untouched(r)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_without_a_device_the_calls_are_refused_loudly():
    q = inputs()
    for r in (_abi.compute_target_double(q["H"], q["lab"], 2),
              _abi.refine_correct_double(q["H"], q["lab"], 2, 0.8),
              _abi.refine_wfit_double(None, q["A"], q["m"], q["n"], q["k"], q["d"], q["H"]),
              _abi.refine_double(None, q["A"], q["m"], q["n"], q["k"], q["W"], q["d"], q["H"], q["lab"], 2, 0.8, 1)):
        assert r["status"] == -1 and "no HIP device" in r["error"]
        sentinel_untouched(r)
    with pytest.raises(_abi.BackendError):
        compute_target(q["H"].T, q["lab"])
    with pytest.raises(_abi.BackendError):
        refine(q["H"].T, labels=q["lab"])
    model = NMFModel(w=q["W"], d=q["d"], h=q["H"].T.copy(), misc={})
    with pytest.raises(_abi.BackendError):
        refine(model, data=q["A"], labels=q["lab"], cycles=1)
