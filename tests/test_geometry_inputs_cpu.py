"""The promises of tests/geometry_inputs.py, proved on the CPU without any kernel: the integer inputs give bitwise-exact fp32
products at every shape the launch-geometry GPU tests use, the real inputs stay inside the derived gamma bound under two
different summation orders, and the dense shapes reach every class and row-tile variant of the table through the library's own
geometry query (host arithmetic: needs no device)."""
import numpy as np
import pytest

from tests import geometry_inputs as gi

F32, F64 = np.float32, np.float64


def test_input_ranges():
    for dt in (F32, F64):
        a = gi.int_array((300, 70), 1, dt)
        assert a.dtype == dt and set(np.unique(a)) == {-2, -1, 0, 1, 2}
        assert set(np.unique(gi.int_array((300, 70), 1, dt, nonneg=True))) == {0, 1, 2, 3}
        r = gi.real_array((100000,), 2, dt)
        assert r.dtype == dt and np.abs(r).min() >= 0.5 and np.abs(r).max() < 2.0 and (r < 0).any() and (r > 0).any()
        assert gi.real_array((1000,), 2, dt, nonneg=True).min() >= 0.5
    assert np.array_equal(gi.int_array((50, 9), 7, F32), gi.int_array((50, 9), 7, F64))          # seeded: the same integers


def _exact_in_fp32(X, Y):
    """fp32 BLAS product == int64 product, and no partial sum in any order can reach 2^24."""
    assert gi.abs_product(X, Y).max() < gi.INT_EXACT_LIMIT
    ref = gi.int_product(X, Y)
    got = X.astype(F32) @ Y.astype(F32)
    assert np.array_equal(got.astype(np.int64), ref) and np.array_equal(got, np.rint(got))
    return ref


def test_int_product_is_the_int64_loop():
    X, Y = gi.int_array((37, 4001), 3, F64), gi.int_array((4001, 19), 4, F64)
    assert np.array_equal(gi.int_product(X, Y), X.astype(np.int64) @ Y.astype(np.int64))


@pytest.mark.parametrize("shape", gi.DENSE_SHAPES, ids=lambda s: "k%d-m%d-n%d" % s)
def test_dense_integer_inputs_are_exact_in_fp32(shape):
    k, m, n = shape
    At = gi.int_array((n, m), 1000 * k + m + n, F32)
    for transposed in (0, 1):
        rows = n if transposed else m
        F = gi.int_array((rows, k), 77 + k + rows + transposed, F32)
        X = At.T if transposed else At
        ref = _exact_in_fp32(X, F)
        cols = np.random.default_rng(5).choice(X.shape[0], size=min(X.shape[0], 16), replace=False)          # the int64 loop itself, sampled
        assert np.array_equal(ref[cols], X[cols].astype(np.int64) @ F.astype(np.int64))


@pytest.mark.parametrize("case", gi.gram_cases(), ids=lambda c: "%s-k%d-r%d%s" % (np.dtype(c[0]).name, c[1], c[2], "-mis" if c[3] else ""))
def test_gram_integer_inputs_are_exact_in_fp32(case):
    dtype, k, r, _ = case
    F = gi.int_array((r, k), k + r, F32)
    _exact_in_fp32(np.ascontiguousarray(F.T), F)


def test_reduction_integer_inputs_are_exact_in_fp32():
    """Row sums of |x|, x and x^2 over the columns (row_norms), and the elementwise products: all integers below 2^24."""
    for dtype, k, c in gi.row_norm_cases():
        X = gi.int_array((c, k), k + c, F32, nonneg=True)
        for term in (X, X * X):
            s = term.sum(axis=0, dtype=F32)
            assert s.max() < gi.INT_EXACT_LIMIT and np.array_equal(s.astype(np.int64), term.astype(np.int64).sum(axis=0))
    for length in gi.sumsq_lengths():
        x = gi.int_array((length,), length, F32)
        assert float((x.astype(F64) ** 2).sum()) < gi.INT_EXACT_LIMIT          # sumsq accumulates in double; exact there a fortiori
    n = gi.elementwise_length()
    x, t = gi.int_array((n,), 1, F32), gi.int_array((n,), 2, F32)
    assert np.array_equal((x + F32(3) * t).astype(np.int64), x.astype(np.int64) + 3 * t.astype(np.int64))


def _sequential_sum(x):
    return np.add.accumulate(x, dtype=x.dtype)[-1]          # accumulate is strictly left to right


@pytest.mark.parametrize("n", [5, 20003, 131077, 1000003])
def test_real_inputs_stay_inside_the_gamma_bound_in_fp32(n):
    """Sequential and pairwise fp32 sums of products of the real inputs against the float64 reference, within gamma_n sum |x y|."""
    x, y = gi.real_array((1, n), n, F32), gi.real_array((n, 1), n + 1, F32)
    ref = gi.hi_product(x, y, F32)
    bound = gi.product_bound(x, y, F32, partials=0)
    prod = (x[0] * y[:, 0]).astype(F32)
    seq, pair = _sequential_sum(prod), prod.sum(dtype=F32)          # numpy's add.reduce is pairwise in blocks of 128
    for got in (seq, pair):
        assert gi.check_real(np.array([[got]]), ref, bound) <= 1.0
    assert seq != pair or n < 200          # the two orders do round differently: the bound is what they share


def test_gamma_and_reference_precision():
    assert gi.gamma(1000, gi.U[F32]) == pytest.approx(1000 * 2.0 ** -24, rel=1e-4)
    assert gi.hi_type(F32) is F64 and gi.hi_type(F64) is np.longdouble
    assert gi.unit_roundoff(np.longdouble) < gi.U[F64] / 1024          # a longdouble that is merely a double would make the fp64 leg vacuous
    X, Y = gi.real_array((40, 3000), 1, F64), gi.real_array((3000, 7), 2, F64)
    assert np.array_equal(gi.hi_product(X, Y, F64, threads=4), X.astype(np.longdouble) @ Y.astype(np.longdouble))
    # an fp64 product accumulated in fp32 is far outside the fp64 bound: the leg sees what integers cannot
    lossy = (X.astype(F32) @ Y.astype(F32)).astype(F64)
    with pytest.raises(AssertionError):
        gi.check_real(lossy, gi.hi_product(X, Y, F64), gi.product_bound(X, Y, F64, 0))
    gi.check_real(X @ Y, gi.hi_product(X, Y, F64), gi.product_bound(X, Y, F64, 0))


def test_sizes_cross_their_thresholds():
    cus = gi.CUS_DEFAULT
    second_trip = [c for c in gi.gram_cases(cus) if c[2] == 20003]
    assert all(32 < gi.gram_nblk(dt, r, cus) < 2 * cus for dt, _, r, _ in second_trip) and len(second_trip) == 6
    capped = [c for c in gi.gram_cases(cus) if c[2] > 100000]
    assert len(capped) == 4 and all(r % 2 == 1 and r > 1.1 * gi.gram_cap_r(dt, cus) and 4 * r < gi.INT_EXACT_LIMIT for dt, _, r, _ in capped)
    for dt, k, c in gi.row_norm_cases(cus):
        assert c % 2 == 1 and 64 < -(-c // 256) and 9 * c < gi.INT_EXACT_LIMIT
    assert max(c for _, _, c in gi.row_norm_cases(cus)) > 1.1 * 2 * cus * 256
    a, b = gi.sumsq_lengths(cus)
    assert 256 < -(-a // 2048) <= 4 * cus < -(-b // 2048) and 4 * b < gi.INT_EXACT_LIMIT
    assert -(-gi.elementwise_length(cus) // 256) > 8 * cus


def test_dense_shapes_reach_every_class_and_row_tile():
    """Through the library's own query: a change of the host rule that loses a class fails here, on the CPU."""
    from rcppml_amd import _abi
    assert _abi.Context.rhs_dense_geometry(_abi.F32, 0, 5, 3, 0) == dict(blocks=0, slices=0, rows_per_slice=0, row_tiles=0)
    with pytest.raises(_abi.BackendError):
        _abi.Context.rhs_dense_geometry(_abi.F32, 10, 10, 129, 0)
    for dtype in (F32, F64):
        dt = _abi.F32 if dtype == F32 else _abi.F64
        for transposed in (0, 1):
            pair = gi.dense_pair(dtype, transposed)
            reached, tiles = set(), set()
            for (k, m, n) in gi.DENSE_SHAPES:
                if pair not in gi.DENSE_EXPECT[(k, m, n)]:
                    assert dtype == F64 and (k, m, n) in gi.DENSE_F32_ONLY
                    continue
                geom = _abi.Context.rhs_dense_geometry(dt, m, n, k, transposed)
                got = gi.dense_classes(geom, dtype, m, n, transposed)
                assert gi.DENSE_EXPECT[(k, m, n)][pair] <= got, (pair, (k, m, n), geom, got)
                reached |= gi.DENSE_EXPECT[(k, m, n)][pair]
                tiles.add(geom["row_tiles"])
            assert reached == set(gi.DENSE_CLASSES), (pair, set(gi.DENSE_CLASSES) - reached)
            assert tiles == gi.DENSE_ROW_TILES[dtype], (pair, tiles)
    k, m, n = gi.DENSE_MISALIGNED
    assert m % 4 == 0          # aligned m: only the base pointer sends the misaligned case to the scalar loads
