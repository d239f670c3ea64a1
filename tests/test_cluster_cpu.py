"""CPU checks of the clustering feature: the numpy restatement of the reference's CPU bipartition() / dclust() (tests/cluster_ref.py,
the GPU path's parity target) against the reference's own known answers, the ABI declarations, the no-device behaviour and the
surface's validation.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cluster_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rcppml_gpu_bipartition_double", "rcppml_gpu_dclust_double", "rcppml_gpu_bipartition_ex", "rcppml_gpu_dclust_ex")


def known_10x10():
    """tests/testthat/test_bipartition.R:6-12 (1-based triplets)."""
    i = [1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10]
    j = [1, 2, 5, 6, 3, 4, 9, 2, 5, 8, 7, 9, 1, 4, 2, 8, 4, 6, 3, 7, 5, 10, 6, 10]
    x = [4, 2, 3, 2, 5, 4, 3, 3, 5, 3, 4, 3, 2, 3, 3, 4, 5, 4, 3, 5, 4, 3, 5, 4]
    return sp.csc_matrix((np.array(x, float), (np.array(i) - 1, np.array(j) - 1)), shape=(10, 10))


def three_blocks(seed=42, per=50, feats=30):
    """test_dclust_expanded.R:140-175: three groups of 50 samples, each high (|N(5, 0.5)|) on its own 10 of 30 features."""
    rng = np.random.default_rng(seed)
    A = np.zeros((feats, 3 * per))
    for g in range(3):
        A[10 * g:10 * (g + 1), per * g:per * (g + 1)] = np.abs(rng.normal(5, 0.5, size=(10, per)))
    return sp.csc_matrix(A), np.repeat(np.arange(3), per)


def test_restatement_known_answer():
    r = R.bipartition(known_10x10(), seed=1, calc_dist=True)
    assert (r["size1"], r["size2"]) == (5, 5)
    assert abs(r["dist"] - 0.137) <= 0.01
    assert len(set(r["samples1"]) & set(r["samples2"])) == 0
    assert sorted(np.concatenate([r["samples1"], r["samples2"]])) == list(range(10))


def test_restatement_initial_w_is_splitmix():
    w = R.init_w(0, 3)                          # seed 0 -> 12345, row 0 gets draws 0..m-1
    from rcppml_amd.data import splitmix64_uniform
    assert np.array_equal(w[0], splitmix64_uniform(12345, 0, 3)) and np.array_equal(w[1], splitmix64_uniform(12345, 3, 3))


def test_restatement_dclust_three_blocks():
    A, labels = three_blocks()
    cl = R.dclust(A, min_samples=10, min_dist=0, seed=42)
    allS = np.sort(np.concatenate([c["samples"] for c in cl]))
    assert np.array_equal(allS, np.arange(A.shape[1]))
    assert len(cl) >= 3
    pur = [np.bincount(labels[c["samples"]]).max() / c["size"] for c in cl]
    assert np.mean(pur) > 0.8


def _check_tree(cl, n):
    ids = [c["id"] for c in cl]
    assert len(set(ids)) == len(ids) and all(set(i) <= {"0", "1"} for i in ids)
    for a in ids:                               # leaves: no id is a prefix of another
        assert not any(b != a and b.startswith(a) for b in ids)
    for c in cl:
        assert np.all(np.diff(c["samples"]) > 0)     # ascending: stable partitions of 0..n-1
    assert np.array_equal(np.sort(np.concatenate([c["samples"] for c in cl])), np.arange(n))
    # emission order = pop order of the LIFO (the "1" child pushed last, popped first): paths in lexicographic order with 1 < 0
    key = [i.translate(str.maketrans("01", "10")) for i in ids]
    assert key == sorted(key)


@pytest.mark.parametrize("min_dist", [0.0, 0.05])
def test_restatement_structure(min_dist):
    A, _ = three_blocks(seed=7)
    splits = []
    cl = R.dclust(A, min_samples=5, min_dist=min_dist, seed=3, splits=splits)
    _check_tree(cl, A.shape[1])
    for s in splits:                            # every split is disjoint, complete and keeps the parent's order
        both = np.concatenate([s["samples1"], s["samples2"]])
        assert np.array_equal(np.sort(both), np.sort(s["parent"]))
        assert np.array_equal(s["samples1"], s["parent"][s["v"] > 0])


def test_restatement_refusals():
    A = known_10x10()
    with pytest.raises(ValueError):
        R.bipartition(A, maxit=0)
    with pytest.raises(ValueError):
        R.dclust(A, min_samples=0)


def _declared():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"RCPPML_GPU_API\s+[\w\s\*]+?\b(rcppml_\w+)\s*\(", src))


def test_header_and_library_carry_the_clustering_entries():
    from rcppml_amd import _abi
    decl = _declared()
    L = _abi.lib()
    for s in NEW_SYMBOLS:
        assert s in decl and s in _abi.EXPORTED_SYMBOLS and hasattr(L, s), s


def test_plugin_signatures_are_the_references():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_bipartition_double", 15), ("rcppml_gpu_dclust_double", 16)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        args = m.group(1)
        assert args.count("*") == count and len(args.split(",")) == count


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    from rcppml_amd import _abi, cluster
    A = known_10x10()
    p, i, x = A.indptr, A.indices, A.data
    part = np.full(10, 7, np.int32)
    v = np.full(10, 7.0)
    center = np.full(20, 7.0)
    r = _abi.bipartition_double(p, i, x, 10, 10, seed=1, partition=part, v=v, center=center)
    assert r["status"] == -1 and r["error"]
    assert np.all(part == 7) and np.all(v == 7.0) and np.all(center == 7.0)        # untouched on failure
    asg = np.full(10, 7, np.int32)
    r = _abi.dclust_double(p, i, x, 10, 10, min_samples=2, assignments=asg)
    assert r["status"] == -1 and r["error"] and np.all(asg == 7)
    assert _abi.bipartition_ex(p, i, x, 10, 10)["status"] == -1
    assert _abi.dclust_ex(p, i, x, 10, 10, min_samples=2)["status"] == -1
    with pytest.raises(_abi.BackendError):
        cluster.bipartition(A)
    with pytest.raises(_abi.BackendError):
        cluster.dclust(A, min_samples=2)


def test_abi_refuses_the_reference_hazards():
    """Refused before any device work, so these hold with or without a GPU."""
    from rcppml_amd import _abi
    A = known_10x10()
    p, i, x = A.indptr, A.indices, A.data
    r = _abi.bipartition_ex(p, i, x, 10, 10, max_iter=0)
    assert r["status"] == -1 and "maxit" in r["error"]
    r = _abi.dclust_ex(p, i, x, 10, 10, min_samples=0)
    assert r["status"] == -1 and "min_samples" in r["error"]
    r = _abi.bipartition_ex(p, i, x, 10, 10, samples=[0, 10])
    assert r["status"] == -1 and "range" in r["error"]
    bad_i = i.copy()
    bad_i[0] = 10
    assert _abi.bipartition_ex(p, bad_i, x, 10, 10)["status"] == -1
    assert _abi.bipartition_ex(p, i, x, 10, 10, seed=-1)["status"] == -1


# a 3 x 2 matrix (p = [0, 2, 3], i = [0, 2, 1]) with one defect each; nnz is the length of x
@pytest.mark.parametrize("p, i, msg", [
    ([1, 2, 3], [0, 2, 1], "col_ptr must start at 0 and end at nnz"),
    ([0, 4, 3], [0, 2, 1], "col_ptr must be non-decreasing"),
    ([0, 2, 3], [0, 3, 1], "row index out of range"),
])
def test_malformed_csc_refusals_are_exact(p, i, msg):
    """Refused before any device work (so with or without a GPU): status -1, this message, nothing written."""
    from rcppml_amd import _abi
    x = np.array([1.0, 2.0, 3.0])
    part, v, center = np.full(2, 7, np.int32), np.full(3, 7.0), np.full(6, 7.0)
    r = _abi.bipartition_double(p, i, x, 3, 2, seed=1, partition=part, v=v, center=center)
    assert (r["status"], r["error"]) == (-1, msg)
    assert np.all(part == 7) and np.all(v == 7.0) and np.all(center == 7.0)
    asg = np.full(2, 7, np.int32)
    r = _abi.dclust_double(p, i, x, 3, 2, min_samples=1, assignments=asg)
    assert (r["status"], r["error"]) == (-1, msg) and np.all(asg == 7)
    r = _abi.bipartition_ex(p, i, x, 3, 2)
    assert (r["status"], r["error"]) == (-1, msg) and r["needed"] == [2, 2, 6]
    r = _abi.dclust_ex(p, i, x, 3, 2, min_samples=1)
    assert (r["status"], r["error"]) == (-1, msg) and (r["clusters"], r["nodes"]) == (2, 4)


def test_surface_validation():
    from rcppml_amd import cluster
    A = known_10x10()
    with pytest.raises(ValueError, match="strictly positive"):
        cluster.bipartition(A, samples=[-1, 2])
    with pytest.raises(ValueError, match="strictly less than the number of columns"):
        cluster.bipartition(A, samples=[0, 10])
    with pytest.raises(ValueError, match="maxit"):
        cluster.bipartition(A, maxit=0)
    with pytest.raises(ValueError, match="min_samples"):
        cluster.dclust(A, min_samples=0)
    with pytest.raises(ValueError, match="maxit"):
        cluster.dclust(A, min_samples=2, maxit=0)
