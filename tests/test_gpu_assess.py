"""GPU checks of the embedding assessment (csrc/ops_assess.hip) against the restatement in tests/assess_ref.py: exact kNN bit for bit
on integer data (every fp32 distance exact, many ties) for the three mask modes, the quirks (NaN points, distances >= 1e30, more than
k duplicates), silhouette / classification / batch outputs bit for bit, k-means on separated blobs, float data against float64,
repeatability, the 26-pointer entry against _ex, and assess() on pbmc3k."""
import os

import numpy as np
import pytest

import assess_ref as R
from rcppml_amd import _abi
from rcppml_amd import assess as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def int_data(n, dim, seed, lo=-3, hi=4):
    return np.random.default_rng(seed).integers(lo, hi, (n, dim)).astype(np.float32)


def check_knn(X, k, mask, group=None, group_k=None, train=None):
    r = _abi.knn_float(X, train, k, mask=mask, group=group, group_k=group_k)
    assert r["status"] == 0, r["error"]
    ri, rd = R.knn(X, train, k, mask=mask, group=group, group_k=group_k)
    assert np.array_equal(r["idx"], ri)
    assert np.array_equal(r["dist"].view(np.int32), rd.view(np.int32))


@pytest.mark.parametrize("dim", [1, 3, 32, 33, 200])
@pytest.mark.parametrize("mask", ["none", "self", "group"])
def test_knn_bitwise_integer_data(dim, mask):
    n = 301 if dim < 100 else 157
    X = int_data(n, dim, dim)
    group = np.random.default_rng(1).integers(0, 5, n) if mask == "group" else None
    for k in (1, 15, 50, n + 3):
        gk = None
        if mask == "group":
            ntr = n - np.bincount(group, minlength=5)
            gk = np.minimum(k, ntr)
        check_knn(X, k, mask, group, gk)


def test_knn_train_matrix_and_large_k():
    X = int_data(700, 8, 3)
    T = int_data(1333, 8, 4)
    check_knn(X, 20, "none", train=T)
    check_knn(X[:40], 300, "none", train=T)          # list of 300: beyond the LDS budget at 32 queries per workgroup


def test_knn_quirks():
    X = int_data(200, 5, 9)
    X[7, 2] = np.nan                                  # every distance to / from point 7 is NaN: never chosen, its list is empty
    X[11] = 1e15                                      # d ~ 1e30 and above: never inserted (-1 slots)
    X[20:40] = X[19]                                  # 21 copies of one point: self can fall out of the first k + 1
    for mask in ("none", "self"):
        for k in (1, 5, 15, 199):
            check_knn(X, k, mask)
    r = _abi.knn_float(X, None, 15, mask="self")
    assert np.all(r["idx"][7] == -1) and np.all(r["dist"][7] == np.float32(1e30))
    assert np.all(r["idx"][11] == -1)


def test_batch_self_exclusion_equals_k_plus_one_with_self():
    # the reference takes k + 1 neighbours including self and drops self: the same set as top-k without self, duplicates included
    X = int_data(150, 4, 5, 0, 2)                     # coordinates in {0, 1}: at most 16 distinct points, many duplicates
    k = 10
    idx_self, _ = R.knn(X, None, k, mask="self")
    idx_all, _ = R.knn(X, None, k + 1, mask="none")
    for i in range(X.shape[0]):
        kept = [j for j in idx_all[i] if j != i][:k]
        assert list(idx_self[i]) == kept
    check_knn(X, k, "self")


def assess_ex(X, labels, nc, batch=None, nb=0, **kw):
    r = _abi.assess_ex(X.astype(np.float64), labels, nc, batch, nb, **kw)
    assert r["status"] == 0, r["error"]
    return r


@pytest.mark.parametrize("dim", [1, 3, 32, 33, 200])
def test_metrics_bitwise_integer_data(dim):
    n = 413 if dim < 100 else 211
    X = int_data(n, dim, 100 + dim)
    rng = np.random.default_rng(dim)
    labels = rng.integers(0, 4, n)
    labels[:2] = 4                                     # a class smaller than the sample count and the fold count
    batch = rng.integers(0, 3, n)
    r = assess_ex(X, labels, 5, batch, 3, clustering=False, spc=37, knn_k=15, folds=5, batch_k=20, seed=11)
    s_pt, s = R.silhouette(X, labels, 5, 37, 11)
    assert np.array_equal(r["sil_point"].view(np.int32), s_pt.view(np.int32))
    assert r["silhouette"] == s
    c = R.classify(X, labels, 5, 15, 5, 11)
    assert np.array_equal(r["fold_ids"], c["fold_ids"])
    assert np.array_equal(r["fold_accuracy"], c["fold_accuracy"], equal_nan=True)
    assert np.array_equal(r["fold_f1"], c["fold_f1"], equal_nan=True)
    assert r["knn_accuracy"] == c["accuracy"] and r["knn_f1"] == c["f1"]
    b = R.batch_mixing(X, batch, 3, 20)
    assert np.array_equal(r["batch_entropy_point"], b["entropy_point"])
    assert np.array_equal(r["batch_sil_point"], b["sil_point"])
    assert r["batch_entropy"] == b["entropy"] and r["batch_sil"] == b["sil"]


def test_metric_edge_cases():
    X = int_data(60, 3, 2)
    labels = np.arange(60) % 3
    for spc in (0, -2, 1):
        r = assess_ex(X, labels, 3, clustering=False, classify=False, batch_mixing=False, spc=spc, seed=5)
        s_pt, s = R.silhouette(X, labels, 3, spc, 5)
        assert np.array_equal(r["sil_point"], s_pt) and r["silhouette"] == s
    # more folds than class members: folds without test points are invalid (NaN), the others average
    r = assess_ex(X, labels, 3, clustering=False, silhouette=False, batch_mixing=False, folds=30, knn_k=4, seed=5)
    c = R.classify(X, labels, 3, 4, 30, 5)
    assert np.array_equal(r["fold_accuracy"], c["fold_accuracy"], equal_nan=True) and r["knn_accuracy"] == c["accuracy"]
    # one point: batch k = min(k, n - 1) = 0 -> entropy and silhouette 0
    r = assess_ex(X[:1], np.zeros(1, int), 1, np.zeros(1, int), 2, clustering=False, silhouette=False, classify=False)
    assert r["batch_entropy"] == 0.0 and r["batch_sil"] == 0.0
    # metrics not asked for stay untouched
    r = _abi.assess_raw(X, labels, 3, np.zeros(60, int), 1, clustering=False, classify=False, init=-5.0)
    assert r["status"] == 0 and r["silhouette"] != -5.0
    assert all(r[k] == -5.0 for k in ("ari", "nmi", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"))


def blobs(n, dim, K, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-10, 10, (K, dim))
    lab = rng.integers(0, K, n)
    return (centers[lab] + spread * rng.standard_normal((n, dim))).astype(np.float32), lab


# seeds whose restarts keep every point's two nearest centroids apart (checked below, not assumed)
@pytest.mark.parametrize("dim,K,seed", [(2, 4, 0), (16, 6, 19), (70, 5, 50)])
def test_kmeans_against_restatement(dim, K, seed):
    X, lab = blobs(613, dim, K, dim)
    nstart, maxiter = 3, 8
    ref = []
    for r in range(nstart):
        asg, gap = R.kmeans(X, K, maxiter, seed, restart=r)
        assert gap > 1e-4, "restart %d: a point's two nearest centroids are within 1e-4 of each other" % r
        ref.append(asg)
    out = assess_ex(X, lab, K, silhouette=False, classify=False, batch_mixing=False, nstart=nstart, maxiter=maxiter, seed=seed)
    aris = [R.ari(lab, a) for a in ref]
    nmis = [R.nmi(lab, a) for a in ref]
    assert np.array_equal(out["restart_ari"], aris) and np.array_equal(out["restart_nmi"], nmis)
    best = int(np.argmax(aris))
    assert np.array_equal(out["assignments"], ref[best])
    assert out["ari"] == aris[best] and out["nmi"] == nmis[best]


def test_kmeans_no_restarts():
    X, lab = blobs(100, 3, 2, 0)
    r = assess_ex(X, lab, 2, silhouette=False, classify=False, batch_mixing=False, nstart=0)
    assert r["ari"] == -1.0 and r["nmi"] == -1.0


def test_float_data_against_float64():
    rng = np.random.default_rng(0)
    n, dim, k = 100000, 32, 15
    X = rng.standard_normal((n, dim)).astype(np.float32)
    qs = np.sort(rng.choice(n, 500, replace=False))
    r = _abi.knn_float(X[qs], X, k)
    assert r["status"] == 0, r["error"]
    X64 = X.astype(np.float64)
    for row, q in enumerate(qs):
        d = ((X64 - X64[q]) ** 2).sum(1)
        order = np.lexsort((np.arange(n), d))
        want, got = order[:k], r["idx"][row]
        if np.array_equal(want, got):
            continue
        # a difference only between candidates whose float64 distances lie within a relative 1e-5
        dk = d[want[-1]]
        for a, b in zip(want, got):
            if a != b:
                assert abs(d[a] - d[b]) <= 1e-5 * max(d[a], d[b]), (q, a, b)
        assert np.all(d[got] <= dk * (1 + 1e-5))


def test_two_runs_are_bitwise_identical():
    X, lab = blobs(3001, 12, 5, 4, spread=2.0)
    batch = np.arange(3001) % 3
    kw = dict(nstart=2, maxiter=10, spc=50, seed=9)
    a = assess_ex(X, lab, 5, batch, 3, **kw)
    b = assess_ex(X, lab, 5, batch, 3, **kw)
    for key in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"):
        assert a[key] == b[key], key
    for key in ("assignments", "sil_point", "batch_entropy_point", "batch_sil_point"):
        assert np.array_equal(a[key], b[key]), key


def test_entry_and_ex_agree():
    X, lab = blobs(900, 7, 3, 8, spread=3.0)
    batch = np.arange(900) % 2
    kw = dict(nstart=3, maxiter=12, spc=40, knn_k=9, folds=4, batch_k=11, seed=-3)
    a = _abi.assess_raw(X, lab, 3, batch, 2, **kw)
    b = assess_ex(X, lab, 3, batch, 2, **kw)
    assert a["status"] == 0
    for key in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy"):
        assert a[key] == b[key], key


def test_ex_capacity_refusal():
    X, lab = blobs(50, 3, 2, 1)
    r = _abi.assess_ex(X, lab, 2, capacity=(49, 10, 5), init=-9.0)
    assert r["status"] == -1 and "point_capacity" in r["error"] and r["ari"] == -9.0


def test_assess_on_pbmc3k():
    from oracle import oracle as O
    from rcppml_amd import cluster, data, svd
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p_, i_, x_ = O.spz_decode(buf)
    A_ = data.CSC((m, n), np.asarray(p_, np.int32), np.asarray(i_, np.int32), np.asarray(x_, np.float64))
    p = svd.pca(A_, k=10, seed=1)
    leaves = cluster.dclust(A_, min_samples=100, seed=1)
    labels = np.zeros(A_.cols, int)
    for c, leaf in enumerate(leaves):
        labels[leaf["samples"]] = c
    batch = np.arange(A_.cols) % 2
    out = A.assess(dict(u=p["v"], d=p["d"]), labels, batch=batch)
    m = out["metrics"]
    for key in ("ari", "nmi", "silhouette", "accuracy_knn", "f1_knn", "batch_silhouette", "batch_knn_entropy"):
        assert np.isfinite(m[key]), key
    assert -1 <= m["ari"] <= 1 and 0 <= m["nmi"] <= 1 and -1 <= m["silhouette"] <= 1
    assert 0 <= m["accuracy_knn"] <= 1 and 0 <= m["f1_knn"] <= 1
    assert 0 <= m["batch_knn_entropy"] <= 1 and -1 <= m["batch_silhouette"] <= 1
    assert m["accuracy_knn"] > 0.5                     # dclust leaves of the same matrix are well separated in its PCA
