"""GPU checks of the similarity entries (csrc/ops_similarity.hip) against the numpy specification (tests/similarity_ref.py) within
its error bounds: the sparse column cosines on shapes placed on the kernel's real boundaries (tile width and wavefronts per
workgroup from rcppml_gpu_cosine_geometry), their edge cases, symmetry and repeatability; the batched dense cosines / correlations;
the refusals on the device; and cosine() / align() end to end.

The kernel tiles the columns of x and deals the columns of y to wavefronts, so every (ny, nx) pair of the shape table is run both
ways round: the tile boundaries and the wavefront boundaries are met on either side."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import similarity_ref as R
from rcppml_amd import _abi
from rcppml_amd import similarity as S
from rcppml_amd.data import CSC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = _abi.cosine_geometry()
T, WAVES = GEO["tile"], GEO["waves"]
NYS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
NXS = [1, WAVES - 1, WAVES, WAVES + 1, 130]
MS = [1, 257, 4097]
DENSITIES = [0.02, 0.5]


def random_csc(m, n, density, seed, signed=True):
    g = np.random.default_rng(seed)
    vals = g.normal(size=(m, n)) if signed else g.uniform(0.1, 1.0, size=(m, n))
    a = sp.csc_matrix(vals * (g.uniform(size=(m, n)) < density))
    a.sort_indices()
    return a


def run(x, y=None, **kw):
    r = _abi.cosine_sparse(CSC.from_scipy(x), None if y is None else CSC.from_scipy(y), **kw)
    assert r["status"] == 0, r["error"]
    return r["C"]


def check(x, y=None, **kw):
    C = run(x, y, **kw)
    ref = R.cosine_sparse_ref(x, y)
    yy = x if y is None else y
    bound = 2 * R.cosine_bound(np.diff(x.indptr), np.diff(yy.indptr))
    err = np.abs(C - ref)
    assert C.shape == ref.shape
    assert np.all(np.isfinite(C))
    assert np.all(err <= bound), (float(err.max()), float((err / bound).max()))
    return C


# ------------------------------------------------------------------------------------------------ sparse entry against the spec
@pytest.mark.parametrize("nx", NXS)
@pytest.mark.parametrize("ny", NYS)
def test_sparse_against_spec(ny, nx):
    for m in MS:
        for density in DENSITIES:
            seed = 7 * ny + 13 * nx + m
            x, y = random_csc(m, nx, density, seed), random_csc(m, ny, density, seed + 1)
            check(x, y)
            check(y, x)              # the tile side and the wavefront side exchanged


def test_sparse_edge_cases():
    m, nx, ny = 300, WAVES + 3, T + 70
    x, y = random_csc(m, nx, 0.2, 1).tolil(), random_csc(m, ny, 0.1, 2).tolil()
    y[40, :] = np.random.default_rng(3).normal(size=ny)      # one all-dense row: more than 64 entries of a row in one tile
    x[40, :] = 1.5
    y[:, 5] = 0                                  # empty columns
    x[:, 1] = 0
    y[17, :] = 0                                 # empty rows
    x[17, :] = 0
    y[:, 9] = 0
    y[33, 9] = 2.5                               # a column with one entry
    x, y = x.tocsc(), y.tocsc()
    x.eliminate_zeros(), y.eliminate_zeros()
    x.sort_indices(), y.sort_indices()
    C = check(x, y)
    assert np.all(C[:, 5] == 0) and np.all(C[1, :] == 0)
    C = check(y, x)                              # the dense row on the tile side
    assert np.all(C[5, :] == 0) and np.all(C[:, 1] == 0)
    # entries only in the last row
    last = sp.csc_matrix((np.array([1.0, -2.0, 3.0]), (np.array([m - 1] * 3), np.array([0, 2, 5]))), shape=(m, 7))
    C = check(last, y)
    assert np.all(C[[1, 3, 4, 6]] == 0)
    C = check(last)
    assert C[0, 2] == -1.0 and C[0, 5] == 1.0 and C[2, 5] == -1.0
    # values spread over twelve orders of magnitude, signed (negative cosines)
    g = np.random.default_rng(4)
    w = random_csc(257, 70, 0.3, 5)
    w.data *= 10.0 ** g.uniform(-6, 6, w.nnz)
    C = check(w, random_csc(257, 66, 0.3, 6))
    assert C.min() < -0.05
    # all-zero inputs: every norm is zero
    z = sp.csc_matrix((20, 5))
    assert np.all(run(z, random_csc(20, 4, 0.5, 7)) == 0) and np.all(run(random_csc(20, 4, 0.5, 7), z) == 0)


@pytest.mark.parametrize("n", [1, 65, T + 1])
def test_y_null_is_symmetric_and_the_xx_call(n):
    x = random_csc(257, n, 0.1, n).tolil()
    if n > 2:
        x[:, 2] = 0                              # a zero column
    x = x.tocsc()
    x.eliminate_zeros()
    x.sort_indices()
    C = check(x)
    assert np.array_equal(C, C.T)
    assert np.array_equal(C, run(x, x))
    nnz = np.diff(x.indptr)
    d = np.diag(C)
    live = nnz > 0
    assert np.all(np.abs(d[live] - 1.0) <= (2 * nnz[live] + 8) * R.U)
    assert np.all(d[~live] == 0.0)


def test_sparse_repeatable_and_independent_of_the_launch():
    x, y = random_csc(4097, 130, 0.05, 11), random_csc(4097, T + 65, 0.05, 12)
    a = run(x, y)
    assert np.array_equal(a, run(x, y))
    assert np.array_equal(a, run(x, y, groups=1))
    assert np.array_equal(a, run(x, y, groups=3))
    b = run(y, x)
    assert np.array_equal(b, run(y, x, groups=1))
    assert np.array_equal(b, a.T)                # the same chains with the roles exchanged


# ------------------------------------------------------------------------------------------------ dense entry
KS = [1, 2, 15, 16, 17, 64, 128]
DENSE_MS = [1, 63, 64, 65, 1000, 2700]


def dense_inputs(reps, m, kx, ky, seed):
    g = np.random.default_rng(seed)
    W = g.normal(size=(reps, m, kx))
    Rm = g.normal(size=(m, ky))
    W[:, :, ::3] += 3.0                          # offset columns: rms / sd about 3
    Rm[:, ::2] = np.abs(Rm[:, ::2])
    return W, Rm


def run_dense(W, Rm, method):
    r = _abi.cosine_dense(np.ascontiguousarray(W.transpose(0, 2, 1)), np.ascontiguousarray(Rm.T), method)
    assert r["status"] == 0, r["error"]
    assert r["launches"] == 3
    return r["sim"]


@pytest.mark.parametrize("ky", KS)
@pytest.mark.parametrize("kx", KS)
def test_dense_against_spec(kx, ky):
    for m in DENSE_MS:
        for reps in (1, 7):
            W, Rm = dense_inputs(reps, m, kx, ky, 31 * kx + 17 * ky + m + reps)
            for method in ("cosine", "cor"):
                got = run_dense(W, Rm, method)
                ref = R.cosine_dense_ref(W, Rm, method)
                kap = 1.0
                if method == "cor":
                    kap = R.kappa(Rm, *W)
                    if m > 1:
                        assert kap <= 16.0
                err = np.abs(got - ref)
                bound = 2 * R.dense_bound(m, kap)
                assert got.shape == (reps, kx, ky) and np.all(np.isfinite(got))
                assert err.max() <= bound, (m, reps, method, float(err.max()), bound)
                if m == 1 and method == "cor":
                    assert np.all(got == 0)      # one row: zero variance everywhere


def test_dense_repeatable_and_replicates_independent():
    for m, kx, ky in ((2700, 17, 16), (65, 128, 64), (1000, 10, 10)):
        W, Rm = dense_inputs(7, m, kx, ky, m + kx)
        for method in ("cosine", "cor"):
            a = run_dense(W, Rm, method)
            assert np.array_equal(a, run_dense(W, Rm, method))
            for q in range(7):
                assert np.array_equal(a[q], run_dense(W[q:q + 1], Rm, method)[0]), (m, method, q)


def test_dense_zero_norm_and_zero_variance():
    W, Rm = dense_inputs(2, 100, 5, 4, 1)
    W[0, :, 1] = 0.0
    Rm[:, 2] = 0.0
    W[1, :, 3] = 2.0                             # constant: zero variance, not zero norm
    c = run_dense(W, Rm, "cosine")
    assert np.all(c[0, 1, :] == 0) and np.all(c[:, :, 2] == 0) and np.all(c[1, 3, [0, 1, 3]] != 0)
    k = run_dense(W, Rm, "cor")
    assert np.all(k[0, 1, :] == 0) and np.all(k[:, :, 2] == 0) and np.all(k[1, 3, :] == 0)
    same = run_dense(Rm[None], Rm, "cor")[0]
    live = [0, 1, 3]
    assert np.all(np.abs(np.diag(same)[live] - 1.0) <= 2 * R.dense_bound(100, R.kappa(Rm)))


# ------------------------------------------------------------------------------------------------ refusals on the device
def test_refusals_leave_outputs_untouched():
    x = CSC.from_scipy(random_csc(50, 6, 0.5, 1))

    def refused(r, word):
        assert r["status"] == -1 and word in r["error"], r["error"]
        assert np.all(r["buffers"][0] == -7.0)

    bad = CSC(x.shape, x.p, x.i, x.x.copy())
    bad.x[3] = np.nan
    refused(_abi.cosine_sparse(bad), "non-finite")
    refused(_abi.cosine_sparse(x, bad), "non-finite")
    uns = CSC(x.shape, x.p, x.i.copy(), x.x)
    s, e = uns.p[0], uns.p[1]
    assert e - s >= 2
    uns.i[s], uns.i[s + 1] = uns.i[s + 1], uns.i[s]
    refused(_abi.cosine_sparse(uns), "strictly increasing")
    refused(_abi.cosine_sparse(x, uns), "strictly increasing")
    refused(_abi.cosine_sparse(x, groups=-1), "groups")
    # an output larger than free memory, requested by dimensions only: nothing is allocated, the small buffer is not written
    n = 400000
    empty = CSC((4, n), np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    refused(_abi.cosine_sparse(empty, out=np.full((4, 4), -7.0, order="F")), "bytes of device memory")
    W = np.ones((1, 129, 10))
    refused(_abi.cosine_dense(W, np.ones((3, 10))), "kx and ky")
    refused(_abi.cosine_dense(np.ones((1, 3, 10)), np.ones((129, 10))), "kx and ky")
    Wn = np.ones((2, 3, 10))
    Wn[1, 2, 9] = np.inf
    refused(_abi.cosine_dense(Wn, np.ones((3, 10))), "non-finite")
    refused(_abi.cosine_dense(np.ones((1, 3, 10)), np.ones((3, 10)), 2), "method")


# ------------------------------------------------------------------------------------------------ end to end
def test_cosine_surface_on_hawaiibirds():
    z = np.load(os.path.join(ROOT, "tests", "golden", "hawaiibirds.npz"))
    A = CSC(z["shape"], z["p"], z["i"], z["x"])
    As = A.to_scipy()
    nnz = np.diff(As.indptr)
    C = S.cosine(A)
    assert np.all(np.abs(C - R.cosine_sparse_ref(As)) <= 2 * R.cosine_bound(nnz, nnz))
    assert np.array_equal(C, C.T) and np.array_equal(C, S.cosine(As))
    sub = As[:, :40].toarray()                                   # two dense inputs of at most 128 columns: the dense entry
    D = S.cosine(sub, As[:, 40:90].toarray())
    assert D.shape == (40, 50)
    assert np.all(np.abs(D - R.cosine_ref(sub, As[:, 40:90])) <= 2 * R.dense_bound(As.shape[0]))
    v = sub[:, 3]
    mv, vm, vv = S.cosine(As, v), S.cosine(v, As), S.cosine(v, sub[:, 4])
    assert mv.shape == (As.shape[1],) and vm.shape == mv.shape and np.isscalar(vv)
    assert np.all(np.abs(mv - R.cosine_ref(As, v)) <= 2 * R.cosine_bound(nnz, [np.count_nonzero(v)])[:, 0])
    assert np.array_equal(vm, mv)                                # deviation 1: the cosine, whichever side the vector is on
    assert abs(vv - R.cosine_ref(v, sub[:, 4])) <= 2 * R.dense_bound(As.shape[0])


def simulate(m, n, k, noise, seed):
    """R/simulateNMF.R:26-70 in structure: every factor owns a block of rows and columns."""
    g = np.random.default_rng(seed)
    w = g.uniform(size=(m, k)) * (g.uniform(size=(m, k)) < 0.3)
    h = g.uniform(size=(k, n)) * (g.uniform(size=(k, n)) < 0.3)
    for f in range(k):
        w[f * m // k:(f + 1) * m // k, f] += 2.0
        h[f, f * n // k:(f + 1) * n // k] += 2.0
    A = w @ h
    return sp.csc_matrix(np.maximum(A + g.normal(0.0, noise * A.mean(), size=A.shape), 0.0))


def permuted(mod, perm):
    from rcppml_amd.nmf import NMFModel
    return NMFModel(mod.w[:, perm].copy(), mod.d[perm].copy(), mod.h[perm, :].copy(), dict(mod.misc))


@pytest.fixture(scope="module")
def fits():
    from rcppml_amd import nmf as N
    A = simulate(120, 100, 5, 0.02, 9)
    return [N.nmf(A, 5, maxit=100, tol=1e-8, seed=s, precision="fp64") for s in range(1, 9)]


@pytest.mark.parametrize("method", ["cosine", "cor"])
def test_align_restores_a_five_cycle(fits, method):
    ref, other = fits[0], fits[1]
    cycle = np.array([1, 2, 3, 4, 0])
    obj = permuted(other, cycle)
    out = S.align(obj, ref, method=method)
    sim = R.cosine_dense_ref(out.w, ref.w)
    assert np.all(np.diag(sim) > 0.99), np.diag(sim)
    order = S.align_order(out.misc["assignment"])
    assert sorted(order) == list(range(5))
    assert np.array_equal(out.w, obj.w[:, order]) and np.array_equal(out.d, obj.d[order]) and np.array_equal(out.h, obj.h[order])
    base = S.align(other, ref, method=method)                    # the unpermuted model lands on the same factors
    assert np.array_equal(out.w, base.w) and np.array_equal(out.d, base.d) and np.array_equal(out.h, base.h)
    rec_in, rec_out = (obj.w * obj.d) @ obj.h, (out.w * out.d) @ out.h
    assert np.allclose(rec_out, rec_in, rtol=0, atol=64 * R.U * np.abs(rec_in).max())      # a sum of 5 terms reordered


def test_align_list_equals_single_calls(fits):
    ref = fits[0]
    g = np.random.default_rng(0)
    objs = [permuted(mod, g.permutation(5)) for mod in fits[1:]]
    assert len(objs) == 7
    many = S.align(objs, ref)
    for mod, got in zip(objs, many):
        one = S.align(mod, ref)
        assert np.array_equal(got.w, one.w) and np.array_equal(got.d, one.d) and np.array_equal(got.h, one.h)
        assert np.array_equal(got.misc["assignment"], one.misc["assignment"])
