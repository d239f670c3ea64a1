"""GPU checks of the sparse cosine kNN entry (cosine_knn_kernel, csrc/kernels_similarity.hip.h) and of cosine_knn() / knn_graph().
Reference: similarity_ref.cosine_sparse_ref, then per column a stable sort by (-value, index).  b = twice cosine_bound of the pair
(idx[r, j], j) the device names (the rank-by-rank comparison would rigorously allow the column's largest bound, no smaller).  nx: one
slot beyond k, one lane row beyond 64, both sides of a tile edge, a third tile; ny: one wavefront, more than a workgroup's eight."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import similarity_ref as R
from rcppml_amd import _abi, nmf as N, similarity as S
from rcppml_amd.data import CSC

pytestmark = pytest.mark.gpu
T = _abi.cosine_geometry()["tile"]
M = 300
SPARSE, FULL = 0.003, 0.5          # about 40 % empty columns and one entry in most others; every pair of columns shares rows
KS = [1, 7, 64]
NXS = ["k+1", 65, T - 1, T + 1, 2 * T + 3]          # ny None below: y = x, run with self excluded and included
CASES = [(nx, ny, d) for nx in NXS for ny in (1, 9, None) for d in (SPARSE, FULL)]


def random_csc(n, density, seed):
    g = np.random.default_rng(seed)
    a = sp.csc_matrix(g.normal(size=(M, n)) * (g.uniform(size=(M, n)) < density))
    a.sort_indices()
    return a


def knn(x, y, k, include_self=False, **kw):
    r = _abi.cosine_knn_sparse(CSC.from_scipy(x), None if y is None else CSC.from_scipy(y), k, include_self, **kw)
    assert r["status"] == 0, r["error"]
    return r["idx"], r["val"]


@functools.lru_cache(maxsize=None)
def inputs(nx, ny, density):
    """x, y (None for y = x), the float64 reference, its bound and the full entry's result on the device: computed once."""
    x = random_csc(nx, density, nx + 7)
    y = None if ny is None else random_csc(ny, density, nx + ny)
    full = _abi.cosine_sparse(CSC.from_scipy(x), None if y is None else CSC.from_scipy(y))
    assert full["status"] == 0, full["error"]
    bound = 2 * R.cosine_bound(np.diff(x.indptr), np.diff((x if y is None else y).indptr))
    return x, y, R.cosine_sparse_ref(x, y), bound, full["C"]


@functools.lru_cache(maxsize=None)
def top64(nx, ny, density, which, skip_self):
    """(idx, val), each (ny, <= 64): every column of inputs()[which] sorted by (-value, index); the first k are the top k."""
    Ct = np.array(inputs(nx, ny, density)[which].T)
    if skip_self:
        np.fill_diagonal(Ct, -np.inf)
    order = np.argsort(-Ct, axis=1, kind="stable")[:, :64]
    return order, np.take_along_axis(Ct, order, axis=1)


def runs(nx, ny, density, k):
    key = (k + 1 if nx == "k+1" else nx, ny, density)
    x, y = inputs(*key)[:2]
    for include_self in ((False, True) if y is None else (True,)):
        yield knn(x, y, k, include_self) + (y is None and not include_self, key)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nx,ny,density", CASES)
def test_against_reference_and_full_entry(nx, ny, density, k):
    for idx, val, skip_self, key in runs(nx, ny, density, k):
        ref, bound = inputs(*key)[2:4]
        cols = np.arange(idx.shape[0])[:, None]
        b = bound[idx, cols]
        assert np.all(np.abs(val - top64(*key, 2, skip_self)[1][:, :k]) <= b)
        assert np.all(np.abs(ref[idx, cols] - val) <= b)
        assert np.all((idx >= 0) & (idx < ref.shape[0])) and all(len(set(row)) == k for row in idx)
        assert not (skip_self and np.any(idx == cols))
        ridx, rval = top64(*key, 4, skip_self)          # the same chain: the bits of the full entry's result, topped on the host
        assert np.array_equal(idx, ridx[:, :k]) and np.array_equal(val.view(np.int64), rval[:, :k].view(np.int64))


def test_planted_ties_and_tile_edges():
    nx = T + 5
    x, y = random_csc(nx, 0.3, 1).tolil(), random_csc(2, 0.3, 2).toarray()
    x[:, nx - 1] = 2.0 * y[:, [0]]                               # the best neighbour in the last slot of the last tile
    x[:, 3] = y[:, [0]] + 0.1 * (np.arange(M)[:, None] % 7 == 0)  # the second best in tile 0 ...
    x[:, T + 1] = x[:, 3]                                        # ... and its exact copy in tile 1
    x[:, 6] = 3.0 * y[:, [1]]                                    # duplicated columns: bitwise equal cosines
    x[:, 9] = x[:, 6]
    x, y = sp.csc_matrix(x), sp.csc_matrix(y)
    assert list(knn(x, y, 2)[0][0]) == [nx - 1, 3]               # the tie at rank k: tile 0 wins
    idx, val = knn(x, y, 64)
    assert list(idx[0, :3]) == [nx - 1, 3, T + 1] and val[0, 1] == val[0, 2]
    assert list(idx[1, :2]) == [6, 9] and val[1, 0] == val[1, 1]


def test_zero_norm_columns():
    x = random_csc(70, SPARSE, 5).tolil()
    x[:, 0] = 0                                                  # a zero-norm column of x and, with y = x, of y
    x[:, 1] = 0
    x[5, :] = 0
    x[5, 1] = x[5, 69] = 1.0                                     # column 1 shares a row with column 69 alone
    idx, val = knn(sp.csc_matrix(x), None, 7)
    assert np.all(val[0] == 0) and list(idx[0]) == list(range(1, 8))          # 0 .. k - 1 minus self
    assert list(idx[1]) == [69, 0, 2, 3, 4, 5, 6] and val[1, 0] > 0 and np.all(val[1, 1:] == 0)


def test_repeatable_and_independent_of_the_launch():
    x, y = random_csc(T + 70, 0.05, 11), random_csc(20, 0.05, 12)
    for yy in (y, None):
        idx, val = knn(x, yy, 15)
        for kw in ({}, {"groups": 1}, {"groups": 3}):
            i2, v2 = knn(x, yy, 15, **kw)
            assert np.array_equal(idx, i2) and np.array_equal(val.view(np.int64), v2.view(np.int64)), kw


def test_refusals_leave_outputs_untouched():
    x = CSC.from_scipy(random_csc(6, 0.5, 1))
    bad = CSC(x.shape, x.p, x.i, x.x.copy())
    bad.x[3] = np.nan
    uns = CSC(x.shape, x.p, x.i.copy(), x.x)
    uns.i[[0, 1]] = uns.i[[1, 0]]
    huge = CSC((2 ** 31 - 1, 4000000), np.zeros(4000001, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for r, word in [(_abi.cosine_knn_sparse(x, k=None), "null"), (_abi.cosine_knn_sparse(bad, k=2), "non-finite"),
                    (_abi.cosine_knn_sparse(x, uns, k=2), "strictly increasing"), (_abi.cosine_knn_sparse(x, k=0), "k must be"),
                    (_abi.cosine_knn_sparse(x, k=65), "k must be"), (_abi.cosine_knn_sparse(x, x, k=7), "eligible"),
                    (_abi.cosine_knn_sparse(x, k=6), "eligible"), (_abi.cosine_knn_sparse(x, k=2, groups=-1), "groups"),
                    (_abi.cosine_knn_sparse(huge, k=2, ny=1), "bytes of device memory")]:
        assert r["status"] == -1 and word in r["error"] and all(np.all(buf == -7) for buf in r["buffers"]), r["error"]
    ok = _abi.cosine_knn_sparse(x, k=6, include_self=True)
    assert ok["status"] == 0 and ok["launches"] == 3          # norms, offsets, the kNN kernel


def test_knn_graph_is_what_the_fit_takes():
    A = sp.csc_matrix(np.abs(random_csc(90, 0.3, 3).toarray()[:60]))
    L = S.knn_graph(A, 5)
    assert L.shape == (90, 90) and np.array_equal(L.toarray(), L.toarray().T)
    mod = N.nmf(A, 4, graph_H=L, graph_lambda=(0, 0.05), seed=1, maxit=10)
    assert np.all(np.isfinite(mod.w)) and np.all(np.isfinite(mod.h)) and np.all(np.isfinite(mod.d))
