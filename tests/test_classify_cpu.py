"""CPU checks of the classifier evaluation: the numpy restatement (tests/classify_ref.py, the GPU path's parity target) on its own,
the surface's messages, split rule and routes, the ABI declarations and the refusals that hold before any device work.  No GPU
needed."""
import os
import re

import numpy as np
import pytest

import classify_ref as CR
from rcppml_amd import _abi, classify as K
from rcppml_amd.data import splitmix64_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the restatement
def brute_auc(y, s):
    """The pair definition: positives i, negatives j, counted when s_i > s_j, or s_i == s_j and i < j."""
    pos, neg = np.flatnonzero(y == 1), np.flatnonzero(y != 1)
    if len(pos) == 0 or len(neg) == 0:
        return 0.5
    cnt = sum(1 for i in pos for j in neg if s[i] > s[j] or (s[i] == s[j] and i < j))
    return cnt / (len(pos) * len(neg))


def test_auc_literal_loop_against_pairs():
    rng = np.random.default_rng(0)
    for trial in range(20):
        n = int(rng.integers(2, 40))
        y = rng.integers(0, 2, n)
        s = rng.integers(0, 4, n) / 4.0 if trial % 2 else rng.random(n)          # every other trial: heavy ties
        assert CR.auc(y, s) == brute_auc(y, s)
    assert CR.auc(np.array([1, 0]), np.array([0.5, 0.5])) == 1.0 and CR.auc(np.array([0, 1]), np.array([0.5, 0.5])) == 0.0
    assert CR.auc(np.ones(5, int), np.arange(5.0)) == 0.5 and CR.auc(np.zeros(5, int), np.arange(5.0)) == 0.5
    assert CR.auc(np.array([], int), np.array([])) == 0.5


def test_metrics_by_hand():
    truth = np.array([0, 0, 1, 1, 2, 2])
    pred = np.array([0, 1, 1, 1, 0, 1])                                           # nobody predicts class 2
    prob = np.eye(3)[pred]
    m = CR.metrics(pred, truth, prob, 3)
    assert m["confusion"].tolist() == [[1, 1, 0], [0, 2, 0], [1, 1, 0]]
    assert m["precision"].tolist() == [0.5, 0.5, 0.0] and m["recall"].tolist() == [0.5, 1.0, 0.0]
    assert m["f1"][2] == 0.0 and m["support"].tolist() == [2, 2, 2] and m["accuracy"] == 0.5
    assert m["weighted_f1"] == pytest.approx((0.5 * 2 + (2 * 0.5 / 1.5) * 2) / 6)
    assert m["auc"].tolist() == [brute_auc((truth == c).astype(int), prob[:, c]) for c in range(3)]


def test_chol_solve_matches_a_dense_solve_and_aliases_a_copy():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 6))
    b, al, ratio = CR.chol_solve(X.T @ X, X.T @ np.ones(50))
    assert not al.any() and 0 < ratio <= 1 and np.allclose(b, np.linalg.solve(X.T @ X, X.T @ np.ones(50)), rtol=1e-10, atol=0)
    X2 = np.hstack([X, X[:, [2]]])                                                # column 6 copies column 2
    b2, al2, _ = CR.chol_solve(X2.T @ X2, X2.T @ np.ones(50))
    assert al2.tolist() == [False] * 6 + [True] and b2[6] == 0.0 and np.allclose(b2[:6], b, rtol=1e-9, atol=0)


OVERLAP = [(257, 3, 3, 33, 0.5, 2), (130, 1, 2, 70, 0.5, 1), (257, 15, 5, 33, 0.5, 1), (96, 3, 2, 1, 0.5, 0), (257, 16, 3, 70, 0.5, 3),
           (257, 17, 2, 33, 0.5, 9)]                      # n_train, p, C, n_test, centre spread (sd), seed
SEPARABLE = [(96, 64, 3, 33, 2.0, 1), (257, 128, 5, 70, 2.0, 1), (130, 17, 17, 33, 2.0, 1), (257, 16, 3, 33, 2.0, 1)]


def case(ntr, p, C, nte, spread, seed):
    x, lab = CR.blobs(ntr + nte, p, C, spread, seed)
    return x[:ntr], x[ntr:], lab[:ntr], lab[ntr:]


def test_gram_against_qr():
    """The measured gap between the two solvers (recorded in classify_ref's docstring).  The bounds: a converging fit at
    cond < 1e2 loses n eps cond ~ 257 x 2.2e-16 x 1e2 = 6e-12; a separable one runs 25 iterations at cond(X'WX) up to 1e4 with
    |beta| growing, where the prototype saw 1.3e-8."""
    for c in OVERLAP:
        tr, te, ltr, lte = case(*c)
        g, q = CR.logistic(tr, te, ltr, lte, c[2], solver="gram"), CR.logistic(tr, te, ltr, lte, c[2], solver="qr")
        gp = np.abs(g["prob"] - q["prob"]).max()
        gb = np.abs(g["coef"] - q["coef"]).max() / np.abs(q["coef"]).max()
        print("overlap", c, "prob gap %.2e beta rel %.2e" % (gp, gb))
        assert g["iters"].tolist() == q["iters"].tolist() and gp <= 1e-11 and gb <= 1e-11
    for c in SEPARABLE:
        tr, te, ltr, lte = case(*c)
        g, q = CR.logistic(tr, te, ltr, lte, c[2], solver="gram"), CR.logistic(tr, te, ltr, lte, c[2], solver="qr")
        gp = np.abs(g["prob"] - q["prob"]).max()
        print("separable", c, "prob gap %.2e cond %.1e" % (gp, g["cond"].max()))
        assert g["iters"].tolist() == [25] * c[2] and not g["converged"].any() and gp <= 1e-7


def test_glm_reaches_the_maximum_likelihood_fit():
    """The converged beta zeroes the score X'(y - mu) (the likelihood equations), to roundoff."""
    tr, te, ltr, lte = case(*OVERLAP[0])
    X = np.hstack([np.ones((tr.shape[0], 1)), tr])
    f = CR.glm_binomial(X, (ltr == 0).astype(float))
    assert f["converged"] == 1 and np.abs(X.T @ ((ltr == 0) - CR.linkinv(X @ f["beta"]))).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------ surface
def _draws(seed, count):
    M, state, out = (1 << 64) - 1, seed, []
    for _ in range(count):
        state = (state + 0x9E3779B97F4A7C15) & M
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        out.append(z ^ (z >> 31))
    return out


@pytest.mark.parametrize("n, frac, seed", [(10, 0.2, 7), (25, 0.5, None), (3, 0.01, 1), (40, 1.0, 3)])
def test_split_rule(n, frac, seed):
    """Partial Fisher-Yates on the SplitMix64 stream, against a hand computation on Python integers."""
    n_test = min(n, max(1, int(round(n * frac))))
    z = _draws(12345 if seed is None else seed, n_test)          # seed None = seed 0, which the project's stream takes as 12345
    idx = list(range(n))
    for i in range(n_test):
        j = min(i + int(np.floor(float(z[i]) / 2.0 ** 64 * (n - i))), n - 1)
        idx[i], idx[j] = idx[j], idx[i]
    got = K.split_indices(n, frac, seed)
    assert got.tolist() == idx[:n_test] and len(set(got.tolist())) == n_test
    assert np.array_equal(splitmix64_uniform(0 if seed is None else seed, 0, n_test), np.array(z, np.float64) / 2.0 ** 64)


@pytest.fixture
def calls(monkeypatch):
    seen = []

    def fake(name):
        def f(*a, **kw):
            seen.append((name, a, kw))
            return dict(status=-1, error="stub: " + name)
        return f
    for name in ("classify_knn", "classify_logistic"):
        monkeypatch.setattr(_abi, name, fake(name))
    return seen


def test_surface_messages_and_routes(calls):
    import rcppml_amd
    assert rcppml_amd.classify_embedding is K.classify_embedding and rcppml_amd.classify_logistic is K.classify_logistic
    assert rcppml_amd.classify_cv is K.classify_cv
    rng = np.random.default_rng(3)
    emb, lab = rng.standard_normal((30, 4)), np.array(list("abc") * 10)
    for f in (K.classify_embedding, K.classify_logistic, K.classify_cv):
        with pytest.raises(ValueError, match=re.escape("length(labels) must equal nrow(embedding)")):
            f(emb, lab[:29])
    assert calls == []
    with pytest.raises(ValueError, match="Fewer training samples than k neighbors"):
        K.classify_embedding(emb, lab, test_idx=np.arange(20), k=15)
    with pytest.raises(ValueError, match="should be one of \"euclidean\", \"cosine\""):
        K.classify_embedding(emb, lab, distance="manhattan")
    with pytest.raises(ValueError, match="classifiers \"rf\" run on R's CPU path and are not available here"):
        K.classify_cv(emb, lab, classifiers=("knn", "rf"))
    assert calls == []                                         # every message comes before any device work
    with pytest.raises(_abi.BackendError, match="stub: classify_knn"):
        K.classify_embedding(emb, lab, k=100, test_fraction=0.01, seed=5, distance="cosine")
    name, a, kw = calls[-1]
    test_idx = K.split_indices(30, 0.01, 5)
    train_idx = np.setdiff1d(np.arange(30), test_idx)
    assert len(test_idx) == 1 and np.array_equal(a[0], emb[train_idx]) and np.array_equal(a[1], emb[test_idx])
    codes = np.arange(30) % 3
    assert np.array_equal(a[2], codes[train_idx]) and np.array_equal(a[3], codes[test_idx])
    assert a[4:] == (3, 29, "cosine")                          # k = min(k, n - 1)
    with pytest.raises(_abi.BackendError, match="stub: classify_logistic"):
        K.classify_logistic(dict(u=emb, d=np.ones(4)), lab, test_idx=[0, 1, 2, 29])
    name, a, kw = calls[-1]
    assert a[0].shape == (26, 4) and a[1].shape == (4, 4) and a[3].tolist() == [0, 1, 2, 2] and a[4] == 3


def test_classify_cv_routes_and_summary(calls):
    rng = np.random.default_rng(4)
    emb, lab = rng.standard_normal((60, 3)), np.arange(60) % 3
    with pytest.raises(_abi.BackendError, match="stub: classify_knn"):
        K.classify_cv(emb, lab, n_folds=4, k_nn=100, seed=9)
    name, a, kw = calls[-1]
    folds = _abi.assess_plan(lab, 3, nstart=0, spc=0, folds=4, seed=9)["fold_ids"]
    tr, te = CR.fold_scale(emb[folds != 0], emb[folds == 0])
    assert np.allclose(a[0], tr, rtol=0, atol=1e-15) and np.allclose(a[1], te, rtol=0, atol=1e-15) and a[5] == tr.shape[0]
    with pytest.raises(_abi.BackendError, match="stub: classify_logistic"):
        K.classify_cv(emb, lab, classifiers="lr")
    rows = [dict(classifier="knn", fold=1, accuracy=0.5, f1=0.25, precision=1.0, recall=0.0, auroc=0.75),
            dict(classifier="lr", fold=1, accuracy=1.0, f1=0.75, precision=0.0, recall=1.0, auroc=float("nan"))]
    s = K.cv_summary(rows)
    assert (s["accuracy_knn"], s["accuracy_lr"], s["accuracy_mean"]) == (0.5, 1.0, 0.75)
    assert s["auroc_mean"] == 0.75 and np.isnan(s["auroc_lr"]) and len(s) == 15


def test_fold_scale_uses_n_minus_1_and_guards_a_zero_sd():
    tr = np.array([[1.0, 5.0], [3.0, 5.0], [5.0, 5.0]])
    a, b = K.fold_scale(tr, np.array([[7.0, 6.0]]))
    assert a[:, 0].tolist() == [-1.0, 0.0, 1.0] and a[:, 1].tolist() == [0.0, 0.0, 0.0] and b.tolist() == [[2.0, 1.0]]


# ------------------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_entries_and_the_library_exports_them():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_classify_metrics_ex", 12), ("rcppml_gpu_classify_knn_ex", 20),
                        ("rcppml_gpu_classify_logistic_ex", 26)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert m.group(1).count("*") == count and len(m.group(1).split(",")) == count, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name), name
    mk = open(os.path.join(ROOT, "rcppml_amd", "csrc", "Makefile")).read()
    assert "ops_classify.hip" in mk


def _inputs():
    rng = np.random.default_rng(5)
    return dict(train=rng.standard_normal((20, 3)), test=rng.standard_normal((4, 3)), train_labels=np.arange(20) % 3,
                test_labels=np.arange(4) % 3, n_classes=3)


def refusal_case(entry, kw):
    """One refused call on pre-filled buffers: the result dict (with its buffers).  Shared with tests/test_gpu_classify.py."""
    a = _inputs()
    kw = dict(kw)
    extra = {}
    for key in ("k", "distance", "maxit", "epsilon"):
        if key in kw:
            extra[key] = kw.pop(key)
    if kw.pop("nan", False):
        a["test"][1, 2] = np.inf
    if kw.pop("bad_label", False):
        a["train_labels"][7] = 3
    if kw.pop("negative_label", False):
        a["test_labels"][0] = -1
    if "dim" in kw:
        d = kw.pop("dim")
        a["train"], a["test"] = np.ones((20, d)), np.ones((4, d))
    a.update(kw)
    if entry == "metrics":
        prob = np.full((4, max(a["n_classes"], 1)), 0.25)
        if a.pop("prob_nan", False):
            prob[0, 0] = np.nan
        return _abi.classify_metrics(prob, a["test_labels"], a["n_classes"])
    f = _abi.classify_knn if entry == "knn" else _abi.classify_logistic
    return f(a["train"], a["test"], a["train_labels"], a["test_labels"], a["n_classes"], **extra)


REFUSALS = [
    ("knn", dict(n_classes=1), "n_classes must be in [2, 256]"),
    ("knn", dict(n_classes=257), "n_classes must be in [2, 256]"),
    ("knn", dict(dim=129), "dim must be in [1, 128]"),
    ("knn", dict(bad_label=True), "train_labels holds a label outside [0, n_classes)"),
    ("knn", dict(negative_label=True), "test_labels holds a label outside [0, n_classes)"),
    ("knn", dict(nan=True), "the test embedding holds a non-finite value"),
    ("knn", dict(k=0), "k must be in [1, n_train]"),
    ("knn", dict(k=21), "k must be in [1, n_train]"),
    ("knn", dict(distance=2), "distance must be 0 (euclidean) or 1 (cosine)"),
    ("logistic", dict(n_classes=1), "n_classes must be in [2, 256]"),
    ("logistic", dict(dim=129), "dim must be in [1, 128]"),
    ("logistic", dict(bad_label=True), "train_labels holds a label outside [0, n_classes)"),
    ("logistic", dict(nan=True), "the test embedding holds a non-finite value"),
    ("logistic", dict(maxit=0), "maxit must be >= 1"),
    ("logistic", dict(epsilon=float("nan")), "epsilon must be finite"),
    ("metrics", dict(n_classes=1), "n_classes must be in [2, 256]"),
    ("metrics", dict(negative_label=True), "test_labels holds a label outside [0, n_classes)"),
    ("metrics", dict(prob_nan=True), "the probability matrix holds a non-finite value"),
]


def untouched(r):
    return all(np.all(b == -7) for b in r["buffers"].values())


@pytest.mark.parametrize("entry, kw, msg", REFUSALS)
def test_abi_refusals_leave_buffers_untouched(entry, kw, msg):
    """Refused before any device work, so these hold with or without a GPU."""
    r = refusal_case(entry, kw)
    assert (r["status"], r["error"]) == (-1, msg)
    assert untouched(r) and len(r["buffers"]) >= 7


def test_abi_refuses_empty_sides():
    a = _inputs()
    r = _abi.classify_knn(a["train"][:0], a["test"], a["train_labels"][:0], a["test_labels"], 3, k=1)
    assert (r["status"], r["error"]) == (-1, "n_train and n_test must be >= 1") and untouched(r)
    r = _abi.classify_logistic(a["train"], a["test"][:0], a["train_labels"], a["test_labels"][:0], 3)
    assert (r["status"], r["error"]) == (-1, "n_train and n_test must be >= 1") and untouched(r)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    a = _inputs()
    for r in (_abi.classify_knn(a["train"], a["test"], a["train_labels"], a["test_labels"], 3),
              _abi.classify_logistic(a["train"], a["test"], a["train_labels"], a["test_labels"], 3),
              _abi.classify_metrics(np.full((4, 3), 1 / 3), a["test_labels"], 3)):
        assert (r["status"], r["error"]) == (-1, "no HIP device") and untouched(r)
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        K.classify_logistic(a["train"], a["train_labels"])
