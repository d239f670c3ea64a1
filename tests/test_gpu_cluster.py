"""GPU clustering path (rcppml_amd/csrc/ops_cluster.hip) against the numpy restatement of the reference's CPU bipartition() /
dclust() (tests/cluster_ref.py).  Before demanding an identical partition every case checks that no sample score of the
restatement sits so close to 0 that the last bits of a reduction order could flip its side."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cluster_ref as R
from oracle import oracle as O
from rcppml_amd import _abi, cluster

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pbmc():
    buf = np.fromfile(os.path.join(HERE, "golden", "pbmc3k.spz"), dtype=np.uint8)
    st, m, n, nnz, vt = O.spz_info(buf)
    assert st == 0
    p, i, x = O.spz_decode(buf)
    return sp.csc_matrix((np.asarray(x, np.float64), np.asarray(i, np.int32), np.asarray(p, np.int32)), shape=(m, n))


def sub(A, r, c):
    S = sp.csc_matrix(A[:r, :c])
    S.sort_indices()
    return S


def parts(A):
    A = sp.csc_matrix(A)
    A.sort_indices()
    return A.indptr, A.indices, A.data


def well_separated(v):
    """Each |v_j| is exactly 0 or clearly away from it (fixture check, not luck)."""
    a = np.abs(np.asarray(v))
    mx = a.max() if a.size else 0.0
    assert np.all((a == 0) | (a > 1e-9 * mx)), np.sort(a[a > 0])[:3]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def groups_matrix(groups, per, feats_per=4, seed=5):
    rng = np.random.default_rng(seed)
    m = groups * feats_per
    rows, cols, vals = [], [], []
    for g in range(groups):
        for s in range(per):
            j = g * per + s
            f = g * feats_per + rng.permutation(feats_per)[:3]
            rows += list(f); cols += [j] * 3; vals += list(rng.uniform(1, 2, 3))
            # a weak shared background feature keeps every split non-degenerate
            rows.append((g * feats_per + feats_per + s % 3) % m); cols.append(j); vals.append(0.05 * rng.uniform(0.5, 1))
    A = sp.coo_matrix((vals, (rows, cols)), shape=(m, groups * per)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A


# ---------------------------------------------------------------------------------------------------------------- bipartition
@pytest.mark.parametrize("shape", [(500, 200), (150, 400)])          # m > n and m < n
def test_bipartition_double_r_shaped(pbmc, shape):
    A = sub(pbmc, *shape)
    m, n = A.shape
    ref = R.bipartition(A, seed=0, calc_dist=True)
    well_separated(ref["v"])
    pad = 16
    part = np.full(n + pad, 9, np.int32)
    v = np.full(m + pad, np.nan)
    center = np.full(2 * m + pad, np.nan)
    r = _abi.bipartition_double(*parts(A), m, n, seed=0.0, partition=part, v=v, center=center)
    assert r["status"] == 0, r["error"]
    side1 = part[:n] == 0
    assert np.array_equal(side1, ref["v"] > 0)
    k = min(m, n)
    assert rel(v[:k], ref["v"][:k]) < 1e-10
    assert np.all(np.isnan(v[k:]))                   # nothing past min(m, n) ... and never past m
    assert np.all(part[n:] == 9) and np.all(np.isnan(center[2 * m:]))
    assert rel(center[:m], ref["center1"]) < 1e-10 and rel(center[m:2 * m], ref["center2"]) < 1e-10
    assert abs(r["dist"] - ref["dist"]) <= 1e-10 * abs(ref["dist"])


def test_known_answer_on_gpu():
    from test_cluster_cpu import known_10x10
    A = known_10x10()
    ref = R.bipartition(A, seed=1)
    well_separated(ref["v"])
    b = cluster.bipartition(A, seed=1)
    assert (b["size1"], b["size2"]) == (5, 5) and abs(b["dist"] - 0.137) <= 0.01
    assert np.array_equal(b["samples1"], ref["samples1"]) and np.array_equal(b["samples2"], ref["samples2"])


@pytest.mark.parametrize("nonneg", [True, False])
def test_bipartition_ex_subset_with_duplicates(pbmc, nonneg):
    A = sub(pbmc, 500, 200)
    rng = np.random.default_rng(3)
    smp = rng.permutation(200)[:120]
    smp = np.concatenate([smp, smp[:15]])            # duplicates, shuffled order
    rng.shuffle(smp)
    ref = R.bipartition(A, smp, seed=11, nonneg=nonneg)
    well_separated(ref["v"])
    r = _abi.bipartition_ex(*parts(A), 500, 200, smp, seed=11.0, nonneg=nonneg)
    assert r["status"] == 0, r["error"]
    assert r["iter"] == ref["iter"]
    assert np.array_equal(r["partition"] == 0, ref["v"] > 0)
    assert rel(r["v"], ref["v"]) < 1e-10
    assert (r["size1"], r["size2"]) == (ref["size1"], ref["size2"])
    assert abs(r["dist"] - ref["dist"]) <= 1e-10 * abs(ref["dist"])
    b = cluster.bipartition(A, samples=smp, seed=11, nonneg=nonneg)
    assert np.array_equal(b["samples1"], ref["samples1"]) and np.array_equal(b["samples2"], ref["samples2"])


def test_bipartition_ex_capacity_is_checked(pbmc):
    A = sub(pbmc, 100, 50)
    r = _abi.bipartition_ex(*parts(A), 100, 50, capacity=(50, 49, 200))
    assert r["status"] == -1 and r["needed"][1] == 50
    r = _abi.bipartition_ex(*parts(A), 100, 50, capacity=(50, 50, 199))
    assert r["status"] == -1 and r["needed"][2] == 200


def test_bipartition_without_calc_dist(pbmc):
    A = sub(pbmc, 300, 120)
    ref = R.bipartition(A, seed=2, calc_dist=False)
    well_separated(ref["v"])
    b = cluster.bipartition(A, seed=2, calc_dist=False)
    assert b["dist"] == -1 and np.all(b["center1"] == 0)
    assert np.array_equal(b["samples1"], ref["samples1"])


# ---------------------------------------------------------------------------------------------------------------- dclust
def _ref_tree(A, **kw):
    splits = []
    cl = R.dclust(A, splits=splits, **kw)
    for s in splits:
        well_separated(s["v"])
    return cl, splits


def _compare(A, cl, kw, centers_tol=1e-12):
    m, n = A.shape
    r = _abi.dclust_ex(*parts(A), m, n, min_samples=kw["min_samples"], min_dist=kw.get("min_dist", 0.0),
                       seed=float(kw.get("seed", 0)))
    assert r["status"] == 0, r["error"]
    assert r["clusters"] == len(cl)
    assert r["ids"] == [c["id"] for c in cl]
    for c, ref in enumerate(cl):
        assert np.array_equal(np.flatnonzero(r["assignments"] == c), ref["samples"])
        assert r["size"][c] == ref["size"]
        assert rel(r["center"][c], ref["center"]) < centers_tol
        if kw.get("min_dist", 0) > 0:
            assert r["radius"][c] == ref["radius"] or abs(r["radius"][c] - ref["radius"]) <= 1e-10 * abs(ref["radius"])
    return r


@pytest.mark.parametrize("min_dist", [0.0, 0.01])
def test_dclust_pbmc_sub(pbmc, min_dist):
    A = sub(pbmc, 500, 200)
    kw = dict(min_samples=50, min_dist=min_dist, seed=0)
    cl, splits = _ref_tree(A, **kw)
    r = _compare(A, cl, kw)
    # R-shaped entry: same assignments; max_clusters truncation
    d = _abi.dclust_double(*parts(A), 500, 200, min_samples=50, min_dist=min_dist)
    assert d["status"] == 0 and d["num_clusters"] == len(cl)
    assert np.array_equal(d["assignments"], r["assignments"])
    if len(cl) > 1:
        t = _abi.dclust_double(*parts(A), 500, 200, min_samples=50, min_dist=min_dist, max_clusters=1)
        assert t["num_clusters"] == 1
        assert np.array_equal(t["assignments"], np.where(r["assignments"] == 0, 0, -1))


@pytest.mark.parametrize("min_dist", [0.0, 0.02])
def test_dclust_pbmc_full(pbmc, min_dist):
    A = sp.csc_matrix(pbmc)
    A.sort_indices()
    kw = dict(min_samples=100, min_dist=min_dist, seed=0)
    cl, splits = _ref_tree(A, **kw)
    r = _compare(A, cl, kw)
    # per-split iteration counts equal the restatement's (node order differs: compare as multisets)
    assert sorted(int(x) for x in r["iter"] if x >= 0) == sorted(s["iter"] for s in splits)


def test_level_batching_equals_single_bipartitions():
    A = groups_matrix(60, 12)
    m, n = A.shape
    kw = dict(min_samples=5, seed=4)
    cl, splits = _ref_tree(A, **kw)
    assert len(cl) >= 30                               # many concurrent clusters per level
    r = _compare(A, cl, kw)
    # each split of the batched tree equals a separate bipartition of the parent's samples
    for s in splits[:40]:
        b = _abi.bipartition_ex(*parts(A), m, n, s["parent"], seed=4.0, calc_dist=False)
        assert b["status"] == 0
        assert np.array_equal(s["parent"][b["partition"] == 0], s["samples1"])
        assert b["iter"] == s["iter"]
    assert r["clusters"] == len(cl)


def test_chunking_gives_the_same_tree(monkeypatch):
    A = groups_matrix(24, 10, seed=9)
    m, n = A.shape
    full = _abi.dclust_ex(*parts(A), m, n, min_samples=4, seed=1.0)
    monkeypatch.setenv("RCPPML_GPU_CLUSTER_BUDGET", str(2 * 32 * m))      # two clusters per launch batch
    small = _abi.dclust_ex(*parts(A), m, n, min_samples=4, seed=1.0)
    assert full["status"] == 0 and small["status"] == 0
    assert full["ids"] == small["ids"] and np.array_equal(full["assignments"], small["assignments"])
    assert np.array_equal(full["center"], small["center"]) and np.array_equal(full["iter"], small["iter"])


def test_degenerate_inputs():
    rng = np.random.default_rng(1)
    D = rng.uniform(size=(30, 40)) * (rng.uniform(size=(30, 40)) < 0.3)
    D[:, [3, 17]] = 0                                   # all-zero columns
    D[[5, 6], :] = 0                                    # empty rows
    A = sp.csc_matrix(D)
    ref = R.bipartition(A, seed=3)
    well_separated(ref["v"])
    b = cluster.bipartition(A, seed=3)
    assert np.array_equal(b["samples1"], ref["samples1"]) and rel(b["v"], ref["v"]) < 1e-10
    # n = 1: h scales to (1, 1), v is rounding noise (1.9e-14 here) and one side is empty: NaN center and dist, as on the CPU
    b = cluster.bipartition(A, samples=[0], seed=3)
    assert b["size1"] + b["size2"] == 1 and np.isnan(b["dist"])
    assert np.all(np.isnan(b["center1"])) == (b["size1"] == 0) and np.all(np.isnan(b["center2"])) == (b["size2"] == 0)
    ref = R.bipartition(A, np.arange(2), seed=3)        # n = 2: v = +-0.998
    b = cluster.bipartition(A, samples=np.arange(2), seed=3)
    assert np.array_equal(b["samples1"], ref["samples1"]) and rel(b["v"], ref["v"]) < 1e-10
    assert abs(b["dist"] - ref["dist"]) <= 1e-10 * ref["dist"]
    ref = R.bipartition(A, seed=3, maxit=1)
    r = _abi.bipartition_ex(*parts(A), 30, 40, seed=3.0, max_iter=1)
    assert r["iter"] == 1 and np.array_equal(r["partition"] == 0, ref["v"] > 0)
    cl = R.dclust(A, min_samples=4, seed=3)
    got = cluster.dclust(A, min_samples=4, seed=3)
    assert [c["id"] for c in got] == [c["id"] for c in cl]
    assert all(np.array_equal(g["samples"], c["samples"]) for g, c in zip(got, cl))


def test_repeat_is_bitwise_identical(pbmc):
    A = sub(pbmc, 500, 200)
    a = _abi.dclust_ex(*parts(A), 500, 200, min_samples=20, min_dist=0.01)
    b = _abi.dclust_ex(*parts(A), 500, 200, min_samples=20, min_dist=0.01)
    assert np.array_equal(a["assignments"], b["assignments"]) and a["ids"] == b["ids"]
    assert np.array_equal(a["center"], b["center"]) and np.array_equal(a["radius"], b["radius"], equal_nan=True)
    x = _abi.bipartition_ex(*parts(A), 500, 200, seed=7.0)
    y = _abi.bipartition_ex(*parts(A), 500, 200, seed=7.0)
    assert np.array_equal(x["v"], y["v"]) and x["dist"] == y["dist"]


def test_surface_dense_equals_sparse(pbmc):
    A = sub(pbmc, 200, 90)
    s = cluster.dclust(A, min_samples=10)
    d = cluster.dclust(A.toarray(), min_samples=10)
    assert [c["id"] for c in s] == [c["id"] for c in d]
    assert all(np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["center"], b["center"]) for a, b in zip(s, d))
    b1 = cluster.bipartition(A, seed=5)
    b2 = cluster.bipartition(A.toarray(), seed=5)
    assert np.array_equal(b1["v"], b2["v"]) and np.array_equal(b1["samples1"], b2["samples1"])
