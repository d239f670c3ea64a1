"""CPU checks of consensus clustering: the declarations / exports of the two entries, the library's host tree
(rcppml_gpu_hclust_average_double) against scipy on tie-free inputs and against the numpy restatement (tests/consensus_ref.py) on tied
ones, hand-worked answers of the restatement itself, the refusals (nothing written, distinct messages), the no-device behaviour and
the Python surface.  No GPU needed."""
import os
import re

import numpy as np
import pytest
from scipy.cluster import hierarchy as H
from scipy.spatial.distance import squareform

import consensus_ref as R
from rcppml_amd import _abi
from rcppml_amd import consensus as CN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcppml_gpu_consensus_double", "rcppml_gpu_hclust_average_double")


def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name in NEW:
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert [a.strip() for a in m.group(1).split(",")][-1] == "int* out_status"


def test_library_exports_the_entries():
    L = _abi.lib()
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name), name


# ------------------------------------------------------------------------------------------------------------ tree vs scipy
def _random_dist(m, seed):
    g = np.random.default_rng(seed)
    D = g.uniform(0.1, 1.0, (m, m))
    D = np.tril(D, -1)
    D = D + D.T
    assert len(np.unique(D[np.tril_indices(m, -1)])) == m * (m - 1) // 2      # tie-free
    return D


def _scipy_sets(Z, m):
    """The two sample sets each scipy step merges."""
    sets = {i: frozenset([i]) for i in range(m)}
    out = []
    for s, row in enumerate(Z):
        a, b = sets[int(row[0])], sets[int(row[1])]
        out.append(frozenset([a, b]))
        sets[m + s] = a | b
    return out


def _merge_sets(merge, m):
    """The same from an R-convention merge matrix."""
    made, out = {}, []
    for s, (a, b) in enumerate(np.asarray(merge)):
        sa = frozenset([-a - 1]) if a < 0 else made[a]
        sb = frozenset([-b - 1]) if b < 0 else made[b]
        out.append(frozenset([sa, sb]))
        made[s + 1] = sa | sb
    return out


def _same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("m", [2, 3, 17, 200, 500])
def test_tree_against_scipy(m):
    D = _random_dist(m, 100 + m)
    y = squareform(D, checks=False)
    Z = H.linkage(y, method="average")
    cuts = sorted({1, 2, min(3, m), min(7, m), m // 2 or 1, m})
    for k_cut in cuts:
        r = _abi.hclust_average_double(D, k_cut)
        assert r["status"] == 0, r["error"]
        np.testing.assert_allclose(r["height"], Z[:, 2], rtol=1e-10, atol=0)
        assert _merge_sets(r["merge"], m) == _scipy_sets(Z, m)
        assert _same_partition(r["clusters"], H.fcluster(Z, k_cut, criterion="maxclust"))
        assert sorted(set(r["clusters"].tolist())) == list(range(1, k_cut + 1))
        if m > 2:
            want = H.cophenet(Z, y)[0]
            print("m=%d k_cut=%d cophenetic %.17g scipy %.17g" % (m, k_cut, r["cophenetic"], want))
            assert abs(r["cophenetic"] - want) <= 1e-10
        else:
            assert np.isnan(r["cophenetic"])           # one pair: no variance


def test_tree_reads_the_lower_triangle_only():
    D = _random_dist(17, 5)
    junk = D.copy()
    junk[np.triu_indices(17, 0)] = np.nan              # as.dist never looks at these
    a, b = _abi.hclust_average_double(D, 4), _abi.hclust_average_double(junk, 4)
    assert b["status"] == 0, b["error"]
    assert np.array_equal(a["merge"], b["merge"]) and np.array_equal(a["height"], b["height"])
    assert np.array_equal(a["clusters"], b["clusters"]) and a["cophenetic"] == b["cophenetic"]


# ------------------------------------------------------------------------------------------------------------ tree vs restatement, ties
def _tied_inputs():
    g = np.random.default_rng(3)
    out = {"all_equal": np.full((9, 9), 0.25)}
    blocks = np.repeat([0, 1], [5, 6])
    out["two_block"] = (blocks[:, None] != blocks[None, :]).astype(np.float64)
    W = [g.uniform(0, 1, (40, 4)) for _ in range(7)]
    out["hard_sevenths"] = 1.0 - R.hard(W)[0]
    return out


@pytest.mark.parametrize("name", ["all_equal", "two_block", "hard_sevenths"])
def test_tree_against_restatement_on_ties(name):
    D = _tied_inputs()[name]
    m = D.shape[0]
    for k_cut in (1, 2, 3, m):
        r = _abi.hclust_average_double(D, k_cut)
        want = R.hclust_average(D, k_cut)
        assert r["status"] == 0, r["error"]
        assert np.array_equal(r["merge"], want["merge"])
        assert np.array_equal(r["height"], want["height"])
        assert np.array_equal(r["clusters"], want["clusters"])
        # numbered by first appearance
        first = [int(np.flatnonzero(r["clusters"] == c)[0]) for c in range(1, k_cut + 1)]
        assert first == sorted(first) and r["clusters"][0] == 1
        if np.isnan(want["cophenetic"]):
            assert np.isnan(r["cophenetic"])
        else:
            assert abs(r["cophenetic"] - want["cophenetic"]) <= 1e-10
    if name == "all_equal":
        assert np.isnan(r["cophenetic"]) and r["status"] == 0
        # every tie goes to the lowest pair: sample 1 with 2, then that cluster with 3, ...
        assert r["merge"][0].tolist() == [-1, -2] and r["merge"][1].tolist() == [-3, 1]
    if name == "two_block":
        assert _abi.hclust_average_double(D, 2)["clusters"].tolist() == [1] * 5 + [2] * 6


# ------------------------------------------------------------------------------------------------------------ hand-worked restatement
def test_hand_worked_hard():
    # replicate 1 labels: 0 0 1 1; replicate 2 labels: 0 1 1 1 (row 0 of replicate 2 is a tie: the first maximum)
    W1 = np.array([[2, 1], [3, 0], [0, 1], [1, 5]], float)
    W2 = np.array([[4, 4], [0, 1], [1, 2], [0, 3]], float)
    cons, lab = R.hard([W1, W2])
    assert lab.tolist() == [[0, 0, 1, 1], [0, 1, 1, 1]]
    assert cons.tolist() == [[1, .5, 0, 0], [.5, 1, .5, .5], [0, .5, 1, 1], [0, .5, 1, 1]]


def test_hand_worked_knn_jaccard():
    # 5 unit vectors in the plane at angles 0, 10, 20, 90, 100 degrees: cosine similarity falls with the angle between them
    ang = np.deg2rad([0, 10, 20, 90, 100])
    W = np.stack([np.cos(ang), np.sin(ang)], 1) * np.array([1, 2, 3, 4, 5])[:, None]     # row scale must not matter
    J, margin, member = R.jaccard(W, 2)
    sets = [set(np.flatnonzero(r).tolist()) for r in member]
    assert sets == [{1, 2}, {0, 2}, {0, 1}, {4, 2}, {3, 2}]
    want = np.eye(5)
    for i in range(5):
        for j in range(5):
            if i != j:
                inter = len(sets[i] & sets[j])
                want[i, j] = inter / (4 - inter)
    # by hand: every pair shares exactly one neighbour except (2, 3) and (2, 4), which share none
    third = 1 / 3
    assert want.tolist() == [[1, third, third, third, third], [third, 1, third, third, third], [third, third, 1, 0, 0],
                             [third, third, 0, 1, third], [third, third, 0, third, 1]]
    assert np.array_equal(J, want)
    assert (margin > 0.1).all()
    cons, _, _ = R.knn_jaccard([W, W[:, ::-1]], 2)      # mirrored: the same angles between the rows
    assert np.array_equal(cons, (want + want) / 2)


def test_knn_clamp_and_build_rules():
    g = np.random.default_rng(0)
    W = g.uniform(0, 1, (6, 3))
    J5, margin, member = R.jaccard(W, 5)
    J9, _, _ = R.jaccard(W, 9)                           # actual_k = m - 1 = 5
    assert np.array_equal(J5, J9) and np.isinf(margin).all()
    assert (member.sum(1) == 5).all()
    off = J5[~np.eye(6, dtype=bool)]
    assert np.all(off == 4 / 6)                          # |Si & Sj| = m - 2 = 4, union = 10 - 4
    # a zero-norm row: similarity 0 to everything; equal similarities go to the lower index
    Z = np.array([[0, 0], [1, 0], [0, 1], [1, 0], [0, 0]], float)
    _, _, member = R.jaccard(Z, 2)
    sets = [set(np.flatnonzero(r).tolist()) for r in member]
    assert sets[0] == {1, 2} and sets[4] == {0, 1}       # all similarities 0: the two lowest other indices
    assert sets[1] == {3, 0} and sets[3] == {1, 0}       # the duplicate first, then the lowest of the zeros
    assert sets[2] == {0, 1}


# ------------------------------------------------------------------------------------------------------------ refusals
def _untouched(r):
    for b in r["buffers"]:
        if isinstance(b, np.ndarray):
            assert np.all(b == -7)
        else:
            assert b == -7.0


def _refused(r, pattern):
    assert r["status"] == -1 and re.search(pattern, r["error"]), r["error"]
    _untouched(r)
    return r["error"]


def test_consensus_refusals_write_nothing():
    W = np.random.default_rng(1).uniform(0, 1, (3, 5, 2))
    msgs = [
        _refused(_abi.consensus_double(None, 5, 2, 3, 0), "null W_stack"),
        _refused(_abi.consensus_double(W[:, :1], 1, 2, 3, 0), "m must be >= 2"),
        _refused(_abi.consensus_double(W, 5, 0, 3, 0), "k must be >= 1"),
        _refused(_abi.consensus_double(W, 5, 2, 0, 0), "reps must be >= 1"),
        _refused(_abi.consensus_double(W, 5, 2, 3, 2), "method must be 0"),
        _refused(_abi.consensus_double(W, 5, 2, 3, -1), "method must be 0"),
        _refused(_abi.consensus_double(W, 5, 2, 3, 1, knn=0), "knn must be >= 1"),
    ]
    for bad in (np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb[2, 4, 1] = bad
        for method in (0, 1):
            msgs.append(_refused(_abi.consensus_double(Wb, 5, 2, 3, method), "non-finite"))
    assert len(set(msgs)) == 7                            # one message per reason (method and non-finite repeat)
    # null output
    st = _abi.C.c_int(-99)
    _abi.lib().rcppml_gpu_consensus_double(_abi._np_ptr(W), _abi._ci(5), _abi._ci(2), _abi._ci(3), _abi._ci(0), _abi._ci(1), None, None,
                                           _abi.C.byref(st))
    assert st.value == -1 and "null out_consensus" in _abi.last_error()


def test_hclust_refusals_write_nothing():
    D = _random_dist(6, 2)
    msgs = [
        _refused(_abi.hclust_average_double(None, 2, m=6), "null dist"),
        _refused(_abi.hclust_average_double(D[:1, :1], 1), "m must be >= 2"),
        _refused(_abi.hclust_average_double(D, 0), r"k_cut must lie in \[1, m\]"),
    ]
    _refused(_abi.hclust_average_double(D, 7), r"k_cut must lie in \[1, m\]")
    for bad in (np.nan, np.inf):
        Db = D.copy()
        Db[4, 1] = bad
        msgs.append(_refused(_abi.hclust_average_double(Db, 2), "non-finite"))
    assert len(set(msgs)) == 4
    st = _abi.C.c_int(-99)
    Df = np.asfortranarray(D)
    _abi.lib().rcppml_gpu_hclust_average_double(_abi._np_ptr(Df), _abi._ci(6), _abi._ci(2), None, None, None, None, _abi.C.byref(st))
    assert st.value == -1 and "null output" in _abi.last_error()


def test_negative_loadings_are_not_refused_for_being_negative():
    W = np.random.default_rng(2).normal(0, 1, (2, 5, 3))
    r = _abi.consensus_double(W, 5, 3, 2, 0)
    if _abi.detect():
        assert r["status"] == 0, r["error"]
    else:
        _refused(r, "no HIP device")


def test_valid_call_without_device():
    """A valid call: refused with nothing written when no device is present; on a device it runs."""
    W = np.random.default_rng(4).uniform(0, 1, (3, 8, 2))
    rs = [_abi.consensus_double(W, 8, 2, 3, 0), _abi.consensus_double(W, 8, 2, 3, 1, knn=3)]
    if _abi.detect():
        assert all(r["status"] == 0 for r in rs)
        return
    for r in rs:
        _refused(r, "no HIP device")
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        CN.consensus_matrix(list(W), "hard")


def test_consensus_nmf_without_device_raises(monkeypatch):
    """No silent CPU path: with the fits stubbed out the consensus stage itself raises BackendError when no device is present (on
    a device the same calls run)."""
    have = bool(_abi.detect())

    class Model:
        def __init__(self, w):
            self.w = w

    g = np.random.default_rng(5)
    calls = []

    def fake(data, k, seed=None, verbose=False, **kw):
        calls.append(dict(seed=seed, verbose=verbose, kw=kw))
        return Model(g.uniform(0, 1, (data.shape[0], k)))

    monkeypatch.setattr(CN._nmf, "nmf", fake)

    def run(**kw):
        if have:
            res = CN.consensus_nmf(np.ones((6, 4)), 2, **kw)
            assert res["consensus"].shape == (6, 6) and len(res["models"]) == kw["reps"]
        else:
            with pytest.raises(_abi.BackendError, match="no HIP device"):
                CN.consensus_nmf(np.ones((6, 4)), 2, **kw)

    run(reps=3, seed=10, tol=1e-3)
    assert [c["seed"] for c in calls] == [11, 12, 13] and all(c["verbose"] is False and c["kw"] == {"tol": 1e-3} for c in calls)
    calls.clear()
    run(reps=2, method="knn")
    assert [c["seed"] for c in calls] == [None, None]


# ------------------------------------------------------------------------------------------------------------ Python surface
def test_python_surface():
    A = np.ones((4, 3))
    with pytest.raises(ValueError, match="'arg' should be one of \"hard\", \"knn_jaccard\""):
        CN.consensus_nmf(A, 2, method="soft")
    with pytest.raises(ValueError, match="'arg' should be one of \"hard\", \"knn_jaccard\""):
        CN.consensus_matrix([A], "x")
    with pytest.raises(NotImplementedError):
        CN.consensus_nmf("/some/where/data.spz", 2)
    with pytest.raises(ValueError, match="all m x k"):
        CN.consensus_matrix([A, np.ones((4, 2))], "hard")
    t = CN.hclust_average(_random_dist(5, 1), 2)           # host only: works without a device
    assert set(t) == {"merge", "height", "clusters", "cophenetic"} and t["merge"].shape == (4, 2)
    with pytest.raises(_abi.BackendError, match="k_cut"):
        CN.hclust_average(_random_dist(5, 1), 9)


@pytest.mark.parametrize("m,k", [(63, 2), (65, 10), (1000, 2), (1000, 64), (2700, 2), (2700, 10)])
def test_random_loadings_have_few_near_ties(m, k):
    """The GPU test screens out rows whose kNN margin is in (0, 1e-9] and allows at most 1 % of them.  For the continuous random
    stacks it draws (standard normal: every direction) the restatement alone excludes none at k >= 10 (smallest margin 3e-7 at
    m = 2700) and at most 0.6 % at k = 2 (15 of 2700 rows at knn = 1: on a circle the cosine is flat between close neighbours, so
    margins near 1e-10 are genuine; uniform positive loadings, a quarter circle, gave 4.5 %)."""
    W = np.random.default_rng(7000 * m + 10 * k + 1).standard_normal((1, m, k))
    for knn in (1, 10):
        _, margins, _ = R.knn_jaccard(list(W), knn, blas=True)
        near = (margins > 0) & (margins <= 1e-9)
        print("m=%d k=%d knn=%d near-tie rows %d smallest margin %.3g" % (m, k, knn, int(near.sum()), margins.min()))
        assert near.mean() <= 0.01
        if k >= 10:
            assert not near.any()
