"""GPU checks of label-guided refinement (rcppml_amd/csrc/ops_refine.hip, rcppml_amd/refine.py) against the numpy restatement
(tests/refine_ref.py).

Tolerance.  Device and restatement differ in summation order only, amplified by the whitening and by the two
solves of a cycle.  For every input the restatement is run twice -- as written, and with the columns visited in reverse order and
all accumulations in long double -- and delta is the largest refine_ref.rel_diff (max |a - b| / max |b|) over the outputs.  The
device gets 100 * max(delta, 2^-52).  delta never sees the device result.  Every case prints delta and the device's deviation.
"""
import functools
import os

import numpy as np
import pytest

import refine_ref as R
from rcppml_amd import _abi
from rcppml_amd import compute_target, refine
from rcppml_amd import nmf as N
from rcppml_amd.data import CSC
from rcppml_amd.refine import as_factor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def bound(delta):
    return 100 * max(delta, EPS)


def emb(k, n, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (k, n))


def check_target(H, codes, C, whiten, tag):
    ref = R.compute_target(H, codes, C, whiten)
    delta = R.rel_diff(R.compute_target(H, codes, C, whiten, variant=True), ref)
    r = _abi.compute_target_double(H.T, codes, C, whiten)
    assert r["status"] == 0, r["error"]
    dev = R.rel_diff(r["target"].T, ref)
    print("compute_target %s: delta %.3e device %.3e bound %.3e" % (tag, delta, dev, bound(delta)))
    assert dev <= bound(delta)
    assert np.array_equal(r["counts"], np.bincount(codes[codes >= 0], minlength=C)[:C])
    return r


@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("C", [1, 2, 7])
@pytest.mark.parametrize("k", [1, 2, 3, 10, 64])
def test_compute_target_parity(k, C, whiten):
    n = 700
    H = emb(k, n, 100 * k + C)
    codes = np.random.default_rng(k + 7 * C).integers(0, C, n).astype(np.int32)
    check_target(H, codes, C, whiten, "k=%d C=%d whiten=%d" % (k, C, whiten))


@pytest.mark.parametrize("whiten", [False, True])
def test_compute_target_empty_class_na_and_floor(whiten):
    n, k = 900, 6
    H = emb(k, n, 5)
    codes = np.random.default_rng(6).integers(0, 5, n).astype(np.int32)
    codes[codes == 2] = 3                                        # class 2 of 5 is empty
    r = check_target(H, codes, 5, whiten, "empty class whiten=%d" % whiten)
    assert r["counts"][2] == 0
    codes = np.random.default_rng(7).integers(-1, 4, n).astype(np.int32)      # -1: NA
    r = check_target(H, codes, 4, whiten, "NA labels whiten=%d" % whiten)
    assert np.array_equal(r["target"][codes < 0], np.zeros(((codes < 0).sum(), k)))
    det = {}
    Hs = H * 1e-6                                                 # the eigenvalue floor of 1e-10 is active
    R.compute_target(Hs, codes, 4, True, detail=det)
    assert det["floored"].any()
    check_target(Hs, codes, 4, whiten, "floored whiten=%d" % whiten)


def test_public_compute_target_takes_any_labels():
    H = emb(5, 300, 8)
    names = np.array(["b", "a", "c"])[np.random.default_rng(9).integers(0, 3, 300)]
    codes, levels = as_factor(names)
    T = compute_target(H, names)
    assert T.shape == (5, 300) and levels == ["a", "b", "c"]
    assert np.array_equal(T, compute_target(H, codes))
    assert np.abs(compute_target(H, np.arange(300) % 3, whiten=False).mean(axis=1)).max() < 1e-10
    some = list(names)
    some[4] = None
    assert np.array_equal(compute_target(H, some)[:, 4], np.zeros(5))


# ------------------------------------------------------------------------------------------------------------------- refine
@functools.lru_cache(maxsize=None)
def fitted(name, k):
    if name == "hawaiibirds":
        z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
        A = CSC(tuple(int(v) for v in z["shape"]), z["p"], z["i"], z["x"])
        dense = A.to_scipy().toarray()
        data = A
    else:
        dense = np.random.default_rng(21).uniform(0, 1, (200, 150)) * (np.random.default_rng(22).uniform(size=(200, 150)) < 0.6)
        data = dense
    model = N.nmf(data, k, seed=42, maxit=20, tol=1e-6, precision="fp64")
    n = dense.shape[1]
    codes = np.random.default_rng(23).integers(0, 5, n).astype(np.int32)
    return data, dense, model, codes


def refine_delta(model, dense, codes, C, lam, cycles, nonneg, whiten=True):
    ref = R.refine(model.w, model.d, model.h, dense, codes, C, lam, cycles, nonneg, whiten)
    var = R.refine(model.w, model.d, model.h, dense, codes, C, lam, cycles, nonneg, whiten, variant=True)
    return ref, max(R.rel_diff(a, b) for a, b in zip(var, ref))


@pytest.mark.parametrize("nonneg", [True, False])
@pytest.mark.parametrize("cycles", [0, 1, 3])
@pytest.mark.parametrize("name,k", [("hawaiibirds", 4), ("hawaiibirds", 10), ("dense", 5)])
def test_refine_parity(name, k, cycles, nonneg):
    data, dense, model, codes = fitted(name, k)
    ref, delta = refine_delta(model, dense, codes, 5, 0.8, cycles, nonneg)
    out = refine(model, data=data, labels=codes, lambda_=0.8, cycles=cycles, nonneg=nonneg)
    devs = [R.rel_diff(a, b) for a, b in zip((out.w, out.d, out.h), (ref[0], ref[1], ref[3]))]
    print("refine %s k=%d cycles=%d nonneg=%d: delta %.3e device W %.3e d %.3e H_corr %.3e bound %.3e" % (
        (name, k, cycles, nonneg, delta) + tuple(devs) + (bound(delta),)))
    if cycles == 0:
        assert np.array_equal(out.w, model.w) and np.array_equal(out.d, model.d)
    assert max(devs) <= bound(delta)
    # the entry's H (before the last correction) too
    m, n = dense.shape
    csc, dn = (data, None) if name == "hawaiibirds" else (None, dense)
    r = _abi.refine_double(csc, dn, m, n, k, model.w, model.d, model.h.T, codes, 5, 0.8, cycles, nonneg, True)
    assert r["status"] == 0, r["error"]
    assert R.rel_diff(r["H"].T, ref[2]) <= bound(delta)
    assert np.array_equal(r["H_corr"].T, out.h)


def test_refine_matrix_input_returns_a_matrix():
    _, dense, model, codes = fitted("hawaiibirds", 4)
    Hc = refine(model.h, labels=codes, lambda_=0.8)
    ref = R.stage1(model.h, codes, 5, 0.8)
    delta = R.rel_diff(R.stage1(model.h, codes, 5, 0.8, variant=True), ref)
    assert isinstance(Hc, np.ndarray) and Hc.shape == model.h.shape and (Hc >= 0).all()
    assert R.rel_diff(Hc, ref) <= bound(delta)
    assert np.abs(refine(model.h, labels=codes, lambda_=0.0) - model.h).max() < 1e-10


def test_refine_batch_path_is_the_composition():
    """refine(batch=...) against: restatement W refit -> the public nmf(target_H, target_lambda=(0, -lambda), maxit=1) -> restatement
    stage 1.  delta is the restatement's own (no batch) on the same inputs and cycles."""
    data, dense, model, codes = fitted("hawaiibirds", 4)
    lam, cycles = 0.8, 2
    n = dense.shape[1]
    batch = np.random.default_rng(31).integers(0, 3, n).astype(np.int32)
    _, delta = refine_delta(model, dense, codes, 5, lam, cycles, True)
    bt = R.compute_target(model.h, batch, 3, whiten=False)
    W, d, H = model.w, model.d, model.h
    Hc = R.stage1(H, codes, 5, lam)
    for _ in range(cycles):
        Wn = R.w_refit(dense, d, Hc, True)
        fit = N.nmf(data, 4, seed=Wn, maxit=1, nonneg=True, target_H=bt, target_lambda=(0.0, -lam), precision="fp64")
        W, d, H = fit.w, fit.d, fit.h
        Hc = R.stage1(H, codes, 5, lam)
    out = refine(model, data=data, labels=codes, batch=batch, lambda_=lam, cycles=cycles)
    devs = [R.rel_diff(a, b) for a, b in zip((out.w, out.d, out.h), (W, d, Hc))]
    print("refine batch: delta %.3e device W %.3e d %.3e H_corr %.3e bound %.3e" % ((delta,) + tuple(devs) + (bound(delta),)))
    assert (out.h >= 0).all() and (out.d > 0).all()
    assert max(devs) <= bound(delta)
    # without cycles the batch has no effect beyond its length check
    assert np.array_equal(refine(model, labels=codes, batch=batch).h, refine(model, labels=codes).h)


# ------------------------------------------------------------------------------------------------------------- repeatability
def test_repeatable_bitwise():
    H = emb(10, 3000, 41)
    codes = np.random.default_rng(42).integers(-1, 7, 3000).astype(np.int32)
    a = _abi.compute_target_double(H.T, codes, 7, True)
    b = _abi.compute_target_double(H.T, codes, 7, True)
    assert a["status"] == 0 and np.array_equal(a["target"], b["target"]) and np.array_equal(a["shift"], b["shift"])
    data, dense, model, lab = fitted("hawaiibirds", 10)
    x = refine(model, data=data, labels=lab, cycles=3)
    y = refine(model, data=data, labels=lab, cycles=3)
    assert np.array_equal(x.w, y.w) and np.array_equal(x.d, y.d) and np.array_equal(x.h, y.h)


def test_what_the_design_promises_about_layout():
    """the class sums depend on the sequence of the LABELLED columns only -- unlabelled columns placed anywhere change
    nothing, bit for bit -- and every column of a class gets the same bits.  Invariance under a permutation of the labelled columns
    is not promised (a column's slot in its chunk decides where it enters the sum)."""
    k, n = 10, 1500
    H = emb(k, n, 43)
    codes = np.random.default_rng(44).integers(0, 4, n).astype(np.int32)
    base = _abi.compute_target_double(H.T, codes, 4, True)
    assert base["status"] == 0
    rng = np.random.default_rng(45)
    at = np.sort(rng.integers(0, n + 1, 400))
    H2 = np.insert(H, at, rng.uniform(size=(k, 400)), axis=1)
    codes2 = np.insert(codes, at, -1)
    wide = _abi.compute_target_double(H2.T, codes2, 4, True)
    assert wide["status"] == 0
    assert np.array_equal(wide["shift"], base["shift"])
    assert np.array_equal(wide["target"][codes2 >= 0], base["target"])
    for c in range(4):
        assert (base["target"][codes == c] == base["shift"][c]).all()


# ------------------------------------------------------------------------------------------------------------------ workflow
def test_guided_workflow_on_hawaiibirds():
    data, dense, model, codes = fitted("hawaiibirds", 4)
    T = compute_target(model.h, codes)
    guided = N.nmf(data, 4, seed=42, maxit=20, target_H=T, target_lambda=0.5)
    for v in (guided.w, guided.d, guided.h):
        assert np.isfinite(v).all() and (v >= 0).all()
    before = R.within_class_cosine(model.h, codes)
    after = R.within_class_cosine(refine(model, labels=codes, lambda_=0.8).h, codes)
    print("within-class cosine: before %.6f after %.6f" % (before, after))
    assert after >= before


def test_a_refused_call_on_the_device_writes_nothing():
    H = emb(3, 50, 46)
    r = _abi.compute_target_double(H.T, np.full(50, 2), 2, True)
    assert r["status"] == -1 and "a label is >= n_classes" in r["error"]
    for b in r["buffers"]:
        assert np.all(b == -7)
    wide = N.NMFModel(w=np.ones((5, 65)), d=np.ones(65), h=np.ones((65, 8)), misc={})
    with pytest.raises(_abi.BackendError, match="k <= 64"):
        refine(wide, data=np.ones((5, 8)), labels=[0, 1] * 4, cycles=1)
