"""GPU checks of the classifier evaluation (rcppml_amd/csrc/ops_classify.hip, rcppml_amd/classify.py) against the numpy restatement
(tests/classify_ref.py).

Tolerances.  A converging logistic fit at cond(X'WX) < 1e2 differs from the restatement's "gram" solver in
summation order only: roundoff of order n eps cond ~ 257 x 2.2e-16 x 1e2 = 6e-12, so beta is held to 1e-10 max|beta|, the
probabilities to 1e-10 and the deviance to 1e-10 relative; the cases are chosen (and asserted, on the restatement alone) so that the
convergence decision has a 10x margin, which makes iters and converged exact.  A separable fit runs all 25 iterations while |beta|
grows; there the probabilities are held to 10x the gap between the restatement's own two solvers on the same input (floor 1e-8).
kNN results are exact: integer coordinates, or generic data whose k-th / (k+1)-th distance gap is asserted to exceed 1e-4 relative
(fp32 distances resolve 1e-6).  Every case prints its figures before it asserts.
"""
import functools
import os

import numpy as np
import pytest

import classify_ref as CR
from rcppml_amd import _abi, classify as K
from test_classify_cpu import OVERLAP, REFUSALS, SEPARABLE, case, refusal_case, untouched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ok(r):
    assert r["status"] == 0, r["error"]
    return r


def same_metrics(r, ref):
    assert np.array_equal(r["predictions"], ref["predictions"])
    assert np.array_equal(r["confusion"], ref["confusion"]) and np.array_equal(r["support"], ref["support"])
    for key in ("precision", "recall", "f1", "auc"):
        assert np.array_equal(r[key], ref[key]), key


@functools.lru_cache(maxsize=None)
def ref_logistic(c, solver):
    tr, te, ltr, lte = case(*c)
    return CR.logistic(tr, te, ltr, lte, c[2], solver=solver)


# ------------------------------------------------------------------------------------------------------------ logistic
@pytest.mark.parametrize("c", OVERLAP)
def test_logistic_overlapping(c):
    tr, te, ltr, lte = case(*c)
    ref = ref_logistic(c, "gram")
    for ratios in ref["ratios"]:
        assert len(ratios) < 25 and ratios[-1] < 1e-9 and (len(ratios) < 2 or ratios[-2] > 1e-7)
    assert ref["converged"].all() and ref["cond"].max() < 1e2 and not ref["aliased"].any()
    r = ok(_abi.classify_logistic(tr, te, ltr, lte, c[2]))
    db = np.abs(r["coef"] - ref["coef"]).max() / np.abs(ref["coef"]).max()
    dp = np.abs(r["prob"] - ref["prob"]).max()
    dd = (np.abs(r["deviance"] - ref["deviance"]) / np.abs(ref["deviance"])).max()
    print("overlap", c, "iters", r["iters"].tolist(), "beta %.2e prob %.2e dev %.2e launches %d" % (db, dp, dd, r["launches"]))
    assert r["iters"].tolist() == ref["iters"].tolist() and r["converged"].tolist() == ref["converged"].tolist()
    assert not r["aliased"].any()
    assert db <= 1e-10 and dp <= 1e-10 and dd <= 1e-10
    same_metrics(r, ref)
    assert r["launches"] == 2 * (int(ref["iters"].max()) + 1) + 3


@pytest.mark.parametrize("c", SEPARABLE)
def test_logistic_separable(c):
    tr, te, ltr, lte = case(*c)
    ref, qr = ref_logistic(c, "gram"), ref_logistic(c, "qr")
    assert ref["iters"].tolist() == [25] * c[2] and not ref["converged"].any()
    bound = max(10 * np.abs(ref["prob"] - qr["prob"]).max(), 1e-8)
    r = ok(_abi.classify_logistic(tr, te, ltr, lte, c[2]))
    dp = np.abs(r["prob"] - ref["prob"]).max()
    print("separable", c, "prob %.2e bound %.2e" % (dp, bound))
    assert r["iters"].tolist() == [25] * c[2] and not r["converged"].any()
    for key in ("coef", "deviance", "prob", "auc", "precision", "recall", "f1"):
        assert np.isfinite(r[key]).all(), key
    assert np.array_equal(r["predictions"], ref["predictions"])
    assert dp <= bound


def degenerate(kind):
    x, lab = CR.blobs(130 + 33, 3, 3, 0.75, 2)
    tr, te, ltr, lte = x[:130].copy(), x[130:].copy(), lab[:130].copy(), lab[130:].copy()
    if kind == "duplicate":
        tr, te = np.hstack([tr, tr[:, [1]]]), np.hstack([te, te[:, [1]]])
    elif kind == "constant":
        tr, te = np.hstack([tr, np.full((130, 1), 2.5)]), np.hstack([te, np.full((33, 1), 2.5)])
    elif kind == "test_only_class":
        lte[::4] = 3                                        # class 3 of 4 has no training row
        return tr, te, ltr, lte, 4
    elif kind == "n_below_P":
        x, lab = CR.blobs(12 + 33, 15, 2, 0.5, 3)
        return x[:12], x[12:], lab[:12], lab[12:], 2
    return tr, te, ltr, lte, 3


@pytest.mark.parametrize("kind", ["duplicate", "constant", "test_only_class", "n_below_P"])
def test_logistic_aliased_and_degenerate(kind):
    tr, te, ltr, lte, C = degenerate(kind)
    ref = CR.logistic(tr, te, ltr, lte, C, solver="gram")
    r = ok(_abi.classify_logistic(tr, te, ltr, lte, C))
    for key in ("coef", "deviance", "prob", "auc"):
        assert np.isfinite(r[key]).all(), key
    dp = np.abs(r["prob"] - ref["prob"]).max()
    print(kind, "iters", r["iters"].tolist(), ref["iters"].tolist(), "aliased", r["aliased"].sum(axis=1).tolist(), "prob %.2e" % dp)
    assert np.array_equal(r["aliased"], ref["aliased"])
    assert r["iters"].tolist() == ref["iters"].tolist() and r["converged"].tolist() == ref["converged"].tolist()
    assert np.array_equal(r["predictions"], ref["predictions"]) and np.array_equal(r["confusion"], ref["confusion"])
    if kind == "n_below_P":
        # 12 rows in 16 columns are separable whatever the labels: the fit follows the separable path (the deviance falls by a
        # constant factor per iteration until the ratio passes 1e-8), so the separable bound applies: 10 x the gap between the
        # restatement's two solvers (floor 1e-8), QR taking the columns the Cholesky kept.  The convergence decision's margin on
        # that path is 12 % on either side, against a roundoff of the deviance of order 1e-7 relative.
        assert all(rt[-1] < 0.9e-8 and rt[-2] > 2e-8 for rt in ref["ratios"]) and np.array_equal(ref["aliased"][0], ref["aliased"][1])
        keep = np.flatnonzero(ref["aliased"][0][1:] == 0)
        qr = CR.logistic(tr[:, keep], te[:, keep], ltr, lte, C, solver="qr")
        bound = max(10 * np.abs(ref["prob"] - qr["prob"]).max(), 1e-8)
        print("n_below_P bound %.2e" % bound)
    else:
        bound = 1e-10 if ref["converged"].all() else 1e-8
    assert dp <= bound
    if kind in ("duplicate", "constant"):
        assert r["aliased"][:, -1].all() and not r["aliased"][:, :-1].any() and np.all(r["coef"][:, -1] == 0.0)
        plain = ok(_abi.classify_logistic(tr[:, :-1], te[:, :-1], ltr, lte, C))            # the fit without the column
        assert np.array_equal(r["predictions"], plain["predictions"])
        assert np.abs(r["prob"] - plain["prob"]).max() <= 1e-10 and np.abs(r["coef"][:, :-1] - plain["coef"]).max() <= 1e-9
    if kind == "test_only_class":
        assert r["support"][3] == len(lte[::4]) and r["recall"][3] == 0.0 and r["converged"][3] == 0


# ------------------------------------------------------------------------------------------------------------ kNN
def integer_case(ntr, p, C, nte, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, (ntr, p)).astype(np.float64), rng.integers(-3, 4, (nte, p)).astype(np.float64),
            rng.integers(0, C, ntr).astype(np.int32), rng.integers(0, C, nte).astype(np.int32))


@pytest.mark.parametrize("ntr, p, C, nte", [(96, 1, 2, 1), (130, 3, 3, 33), (257, 17, 17, 70), (257, 128, 5, 33), (130, 64, 5, 70)])
def test_knn_exact_inputs(ntr, p, C, nte):
    """Small integer coordinates: the fp32 squared distances are exact and many tie, so the order falls to the train index."""
    tr, te, ltr, lte = integer_case(ntr, p, C, nte, ntr + p)
    for k in (1, 5, 15, ntr):
        ref = CR.knn(tr, te, ltr, lte, C, k)
        r = ok(_abi.classify_knn(tr, te, ltr, lte, C, k))
        assert np.array_equal(r["votes"], ref["votes"]), k
        same_metrics(r, ref)
        assert r["launches"] == 5


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
@pytest.mark.parametrize("ntr, p, C, nte, k", [(257, 3, 3, 70, 5), (130, 16, 5, 33, 15), (96, 15, 2, 33, 1)])
def test_knn_generic_data(ntr, p, C, nte, k, distance):
    ref = None
    for seed in range(200):                             # the first seed whose every row has a clear k-th / (k+1)-th gap
        x, lab = CR.blobs(ntr + nte, p, C, 1.0, seed)
        x = x + 0.5                                     # off-centre, so the cosine rows are not degenerate
        cand = CR.knn(x[:ntr], x[ntr:], lab[:ntr], lab[ntr:], C, k, distance)
        if cand["gap"].min() > 1e-4:
            ref = cand
            break
    assert ref is not None and ref["gap"].min() > 1e-4
    r = ok(_abi.classify_knn(x[:ntr], x[ntr:], lab[:ntr], lab[ntr:], C, k, distance))
    print("knn", distance, (ntr, p, C, nte, k), "seed", seed, "min gap %.2e" % ref["gap"].min())
    assert np.array_equal(r["votes"], ref["votes"])
    same_metrics(r, ref)


def test_metrics_entry_with_ties_and_an_unpredicted_class():
    rng = np.random.default_rng(8)
    prob = rng.integers(0, 4, (300, 5)) / 4.0           # heavy ties; 300 rows: two blocks of the pair count
    prob[:, 4] = -1.0                                   # never the maximum
    truth = rng.integers(0, 5, 300).astype(np.int32)
    pred = np.array([CR.which_max(row) for row in prob])
    ref = CR.metrics(pred, truth, prob, 5)
    r = ok(_abi.classify_metrics(prob, truth, 5))
    same_metrics(r, ref)
    assert r["precision"][4] == 0.0 and r["support"][4] > 0
    r = ok(_abi.classify_metrics(prob[:7], np.zeros(7, np.int32), 5))            # an empty side: 0.5
    assert r["auc"].tolist() == [0.5] * 5


# ------------------------------------------------------------------------------------------------------------ determinism
def test_two_calls_and_a_halved_grid_are_bitwise_equal():
    c = OVERLAP[2]                                      # 257 rows: 3 chunks
    tr, te, ltr, lte = case(*c)
    a = ok(_abi.classify_logistic(tr, te, ltr, lte, c[2]))
    for rb in (0, 2, 1):
        b = ok(_abi.classify_logistic(tr, te, ltr, lte, c[2], row_blocks=rb))
        for key in ("coef", "prob", "deviance", "iters", "converged", "auc", "confusion"):
            assert a[key].tobytes() == b[key].tobytes(), (rb, key)
    k1 = ok(_abi.classify_knn(tr, te, ltr, lte, c[2], 5))
    k2 = ok(_abi.classify_knn(tr, te, ltr, lte, c[2], 5))
    assert k1["votes"].tobytes() == k2["votes"].tobytes() and k1["auc"].tobytes() == k2["auc"].tobytes()


@pytest.mark.parametrize("entry, kw, msg", REFUSALS)
def test_refusals_on_the_device(entry, kw, msg):
    r = refusal_case(entry, kw)
    assert (r["status"], r["error"]) == (-1, msg) and untouched(r)


# ------------------------------------------------------------------------------------------------------------ surface
def test_classify_cv_details():
    x, lab = CR.blobs(150, 6, 3, 0.75, 4)
    out = K.classify_cv(x, lab, n_folds=5, k_nn=15, seed=42)
    rows = CR.classify_cv(x, lab, 3, out["fold_ids"], 5)
    assert [(d["classifier"], d["fold"]) for d in out["details"]] == [(d["classifier"], d["fold"]) for d in rows] and len(rows) == 10
    for d, e in zip(out["details"], rows):
        for m in K.CV_METRICS:
            assert abs(d[m] - e[m]) <= 1e-10, (d["classifier"], d["fold"], m)
    assert out["metrics"] == K.cv_summary(out["details"]) and len(out["metrics"]) == 15
    assert out["metrics"]["accuracy_mean"] == pytest.approx(np.mean([e["accuracy"] for e in rows]), abs=1e-10)


def test_surface_on_hawaiibirds():
    from rcppml_amd import cluster, nmf as N
    from rcppml_amd.data import CSC
    z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
    A = CSC(tuple(int(v) for v in z["shape"]), z["p"], z["i"], z["x"])
    model = N.nmf(A, 6, seed=42, maxit=20, tol=1e-6, precision="fp64")
    n = int(z["shape"][1])
    labels = np.zeros(n, np.int64)
    for ci, leaf in enumerate(cluster.dclust(A, min_samples=150, seed=1)):
        labels[leaf["samples"]] = ci
    C = int(labels.max()) + 1
    assert C >= 2
    emb = (np.asarray(model.d)[:, None] * np.asarray(model.h)).T
    names = np.array(["grid%02d" % v for v in labels])
    for out in (K.classify_embedding(emb, names, k=5, seed=3), K.classify_logistic(emb, names, seed=3)):
        nt = len(out["test_idx"])
        assert nt == round(0.2 * n) and len(out["train_idx"]) == n - nt and out["n_classes"] == C
        assert out["confusion"].sum() == nt and out["confusion"].shape == (C, C)
        assert out["accuracy"] == np.trace(out["confusion"]) / nt
        assert np.array_equal(out["test_labels"], names[out["test_idx"]])
        assert 0.0 <= out["auc"] <= 1.0 and 0.0 <= out["macro_f1"] <= 1.0
        assert out["per_class"]["support"].sum() == nt and list(out["per_class"]["class"]) == sorted(set(names))
    assert out["method"] == "logistic" and out["coef"].shape == (C, 7) and np.isfinite(out["prob"]).all()
    codes = np.unique(names, return_inverse=True)[1]
    ref = CR.knn(emb[out["train_idx"]], emb[out["test_idx"]], codes[out["train_idx"]], codes[out["test_idx"]], C, 5)
    knn = K.classify_embedding(emb, names, k=5, test_idx=out["test_idx"])
    agree = np.mean(knn["predictions"] == np.unique(names)[ref["predictions"]])
    print("hawaiibirds kNN agreement with float64", agree, "accuracy", knn["accuracy"])
    assert agree >= 0.99                                 # fp32 distances: a near-tie may fall the other way
