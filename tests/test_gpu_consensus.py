"""GPU checks of consensus clustering: rcppml_gpu_consensus_double (csrc/ops_consensus.hip) against the numpy restatement
(tests/consensus_ref.py), bitwise for "hard" and, for "knn_jaccard", neighbour sets equal on every row that is not a genuine near-tie
(and bitwise when there is none); the build's two rules on zero-norm and duplicated rows; repeatability; refusals on the device; and
consensus_nmf end to end on planted clusters and on hawaiibirds."""
import os

import numpy as np
import pytest

import consensus_ref as R
from rcppml_amd import _abi
from rcppml_amd import consensus as CN
from rcppml_amd.data import CSC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_TIE = 1e-9          # sims are O(1) in fp64; device and numpy dot products differ near 1e-16
MS = [2, 63, 64, 65, 1000, 2700]
KS = [1, 2, 10, 64]
REPS = [1, 7, 50]


def stack(reps, m, k, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (reps, m, k))


@pytest.mark.parametrize("reps", REPS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
def test_hard_bitwise(m, k, reps):
    W = stack(reps, m, k, 1000 * m + 10 * k + reps)
    r = _abi.consensus_double(W, m, k, reps, "hard")
    assert r["status"] == 0, r["error"]
    cons, lab = R.hard(list(W))
    assert np.array_equal(r["labels"], lab)
    assert np.array_equal(r["consensus"], cons)
    assert np.all(r["consensus"].diagonal() == 1.0)


def test_hard_argmax_ties_go_to_the_first():
    W = stack(7, 65, 10, 3)
    W[:, :, 6] = W[:, :, 2]                      # a duplicated column
    W[:, ::2, 2] = 2.0                           # ... that holds the maximum in every other row
    W[:, ::2, 6] = 2.0
    W[:, 1::4, :] = 0.5                          # and rows that are constant: the first column
    r = _abi.consensus_double(W, 65, 10, 7, "hard")
    assert r["status"] == 0, r["error"]
    cons, lab = R.hard(list(W))
    assert (r["labels"][:, ::2] == 2).all() and (r["labels"][:, 1::4] == 0).all()
    assert np.array_equal(r["labels"], lab) and np.array_equal(r["consensus"], cons)


def device_sets(W1, m, k, knn):
    """J of one replicate alone: entry (i, j) depends on the neighbour sets of i and j only."""
    r = _abi.consensus_double(W1[None], m, k, 1, "knn_jaccard", knn=knn)
    assert r["status"] == 0, r["error"]
    return r["consensus"]


def check_knn(W, knn, blas=True):
    """Neighbour sets equal the restatement's on every row that is not a genuine near-tie (0 < margin <= 1e-9; at most 1 % of the
    rows); exact ties (margin 0) are decided by the rule and compared like any other row.  Sets are compared a replicate at a time
    through the device's single-replicate J: row i of J is determined by the sets, and J[i, :] == ref for all rows with equal sets.
    When no row is excluded the consensus of the whole stack is bitwise the restatement's."""
    reps, m, k = W.shape
    cons, margins, members = R.knn_jaccard(list(W), knn, blas=blas)
    near = (margins > 0) & (margins <= NEAR_TIE)
    print("m=%d k=%d reps=%d knn=%d: near-tie rows %d of %d, smallest positive margin %.3g" % (
        m, k, reps, knn, int(near.sum()), near.size, margins[margins > 0].min() if (margins > 0).any() else np.inf))
    assert near.mean() <= 0.01
    r = _abi.consensus_double(W, m, k, reps, "knn_jaccard", knn=knn)
    assert r["status"] == 0, r["error"]
    assert r["labels"] is None
    if not near.any():
        assert np.array_equal(r["consensus"], cons)
        return
    # some rows are near-ties: compare replicate by replicate, on the rows and columns that are not
    for q in range(reps):
        Jd = device_sets(W[q], m, k, knn)
        Jr, _, _ = R.jaccard(W[q], knn, blas=blas)
        ok = ~near[q]
        assert np.array_equal(Jd[np.ix_(ok, ok)], Jr[np.ix_(ok, ok)])


def normal_stack(reps, m, k, seed):
    """Every direction, not only the positive orthant: at k = 2 positive loadings lie on a quarter circle, where the cosine is so
    flat between close neighbours that more than 1 % of the rows of a 2700-sample replicate are genuine near-ties."""
    return np.random.default_rng(seed).standard_normal((reps, m, k))


def knn_values(m):
    return sorted({1, 10, m - 1, m + 5})


@pytest.mark.parametrize("reps", REPS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("m", MS)
def test_knn_jaccard(m, k, reps):
    W = normal_stack(reps, m, k, 7000 * m + 10 * k + reps)
    for knn in knn_values(m):
        check_knn(W, knn)


def test_knn_build_rules_zero_norm_and_duplicates():
    g = np.random.default_rng(11)
    W = g.uniform(0.05, 1.0, (7, 130, 10))
    W[:, [0, 17, 64, 129], :] = 0.0              # zero-norm rows: similarity 0 to everything
    W[:, 40:50, :] = W[:, 39:40, :]              # exactly duplicated rows: exact ties, the lower index first
    W[:, 100, :] = W[:, 3, :] * 2.0              # a scaled copy: the same direction (power of two: exact)
    for knn in (1, 5, 10, 128, 129):
        cons, margins, _ = R.knn_jaccard(list(W), knn)           # the exact-order similarity: ties are exact in the restatement
        assert (margins == 0).any() or knn >= 129
        r = _abi.consensus_double(W, 130, 10, 7, "knn_jaccard", knn=knn)
        assert r["status"] == 0, r["error"]
        assert not ((margins > 0) & (margins <= NEAR_TIE)).any()
        assert np.array_equal(r["consensus"], cons)
    # negative loadings are accepted
    Wn = g.normal(0, 1, (3, 65, 4))
    for method, knn in (("hard", 1), ("knn_jaccard", 6)):
        r = _abi.consensus_double(Wn, 65, 4, 3, method, knn=knn)
        assert r["status"] == 0, r["error"]
        assert np.array_equal(r["consensus"], R.consensus(list(Wn), method, knn))


def test_two_runs_are_bitwise_identical():
    W = stack(7, 1000, 10, 5)
    for method in ("hard", "knn_jaccard"):
        a = _abi.consensus_double(W, 1000, 10, 7, method, knn=10)
        b = _abi.consensus_double(W, 1000, 10, 7, method, knn=10)
        assert a["status"] == 0 and b["status"] == 0
        assert a["consensus"].tobytes() == b["consensus"].tobytes()
        assert np.array_equal(a["consensus"], a["consensus"].T)
    D = 1.0 - a["consensus"]
    t1, t2 = _abi.hclust_average_double(D, 10), _abi.hclust_average_double(D, 10)
    for key in ("merge", "height", "clusters"):
        assert t1[key].tobytes() == t2[key].tobytes()
    assert t1["cophenetic"] == t2["cophenetic"]


def test_refused_call_on_the_device_writes_nothing():
    W = stack(3, 8, 2, 9)
    Wb = W.copy()
    Wb[1, 2, 0] = np.nan
    for r in (_abi.consensus_double(Wb, 8, 2, 3, "hard"), _abi.consensus_double(W, 8, 2, 3, 5), _abi.consensus_double(W, 8, 2, 3, 1, knn=0),
              _abi.consensus_double(W, 1, 2, 3, 0)):
        assert r["status"] == -1 and r["error"]
        assert all(np.all(b == -7) for b in r["buffers"])
    ok = _abi.consensus_double(W, 8, 2, 3, "hard")             # the device still works afterwards
    assert ok["status"] == 0 and np.array_equal(ok["consensus"], R.hard(list(W))[0])


# ------------------------------------------------------------------------------------------------------------ end to end
def planted(m_per=40, k=3, n=60, seed=0):
    """Well-separated row clusters: each cluster loads one block of features, plus a little noise."""
    g = np.random.default_rng(seed)
    truth = np.repeat(np.arange(k), m_per)
    per = n // k
    A = g.uniform(0.0, 0.05, (k * m_per, n))
    for c in range(k):
        A[np.ix_(truth == c, np.arange(c * per, (c + 1) * per))] += g.uniform(1.0, 2.0, (m_per, per))
    perm = g.permutation(k * m_per)
    return A[perm], truth[perm]


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def check_end_to_end(A, k, method, knn, reps, seed):
    res = CN.consensus_nmf(A, k, reps=reps, method=method, knn=knn, seed=seed, maxit=30, tol=1e-4)
    Ws = [np.asarray(mod.w, np.float64) for mod in res["models"]]
    assert len(Ws) == reps and res["k"] == k and res["reps"] == reps and res["method"] == method
    if method == "hard":
        assert res["knn"] is None
        assert np.array_equal(res["consensus"], R.hard(Ws)[0])
    else:
        assert res["knn"] == knn
        check_knn(np.stack(Ws), knn, blas=False)
        cons, margins, _ = R.knn_jaccard(Ws, knn)
        if not ((margins > 0) & (margins <= NEAR_TIE)).any():
            assert np.array_equal(res["consensus"], cons)
    assert sorted(set(res["clusters"].tolist())) == list(range(1, k + 1))
    assert -1.0 <= res["cophenetic"] <= 1.0
    assert res["merge"].shape == (A.shape[0] - 1, 2) and res["height"].shape == (A.shape[0] - 1,)
    again = CN.consensus_nmf(A, k, reps=reps, method=method, knn=knn, seed=seed, maxit=30, tol=1e-4)
    assert again["consensus"].tobytes() == res["consensus"].tobytes()
    assert np.array_equal(again["clusters"], res["clusters"]) and again["cophenetic"] == res["cophenetic"]
    assert np.array_equal(again["merge"], res["merge"]) and np.array_equal(again["height"], res["height"])
    return res, Ws


@pytest.mark.parametrize("method", ["hard", "knn_jaccard"])
def test_end_to_end_planted(method):
    A, truth = planted()
    res, Ws = check_end_to_end(A, 3, method, 10, 10, 42)
    # the separation is a property of the input: the restatement on the same models recovers the planted partition
    ref_tree = R.hclust_average(1.0 - R.consensus(Ws, method, 10), 3)
    assert same_partition(ref_tree["clusters"], truth)
    assert same_partition(res["clusters"], truth)


@pytest.mark.parametrize("method", ["hard", "knn_jaccard"])
def test_end_to_end_hawaiibirds(method):
    z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
    A = CSC(z["shape"], z["p"], z["i"], z["x"]).to_scipy()
    check_end_to_end(A, 6, method, 10, 7, 1)
