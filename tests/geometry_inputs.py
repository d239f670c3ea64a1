"""Inputs, references and derived error bounds for the launch-geometry tests (tests/test_gpu_dense_matrix.py,
tests/test_gpu_reduction_geometry.py); tests/test_geometry_inputs_cpu.py proves on the CPU, without any kernel, that they keep
their promises.

Two kinds of input:

* exact-integer: seeded integers in {-2..2} ({0..3} where an op needs nonnegative data).  With a reduction of at most 4e6 terms
  (1.8e6 for products of two {0..3} operands) every partial sum of products is an integer below 2^24, so fp32 and fp64 results
  are exact in ANY summation order, with or without FMA.  The reference is the int64 product and the assertion is bitwise
  equality: this is the leg that notices one dropped, doubled or misplaced term at any size.
* real-valued: magnitudes in [0.5, 2) with random signs (no subnormals).  The bound is derived, entrywise:
  |got - ref|_ab <= (gamma_n(u) + gamma_n(u_ref)) (|X| |Y|)_ab with gamma_n(u) = n u / (1 - n u), u = 2^-24 (fp32) or 2^-53 (fp64),
  n = reduction length + number of partial sums added + 4, and the reference in float64 for fp32 and np.longdouble for fp64
  (u_ref its unit roundoff: the reference's own error, a 2^-11 .. 2^-29 part of the bound).  This leg catches a loss of
  precision integers cannot show (an fp64 path accumulating in fp32); it is not the leg that finds dropped terms."""
import concurrent.futures as cf

import numpy as np

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
INT_EXACT_LIMIT = 2 ** 24
CUS_DEFAULT = 256          # MI355X; the GPU tests read the device's count, the CPU proof uses this one


def hi_type(dtype):
    """The reference precision of the real-valued leg."""
    return np.float64 if dtype == np.float32 else np.longdouble


def unit_roundoff(t):
    return U[t] if t in U else float(np.finfo(t).eps) / 2


def gamma(n, u):
    assert n * u < 0.5
    return n * u / (1.0 - n * u)


def int_array(shape, seed, dtype, nonneg=False):
    """Seeded integers in {-2..2} (nonneg: {0..3}) as `dtype`."""
    rng = np.random.default_rng(seed)
    lo, hi = (0, 4) if nonneg else (-2, 3)
    return rng.integers(lo, hi, size=shape, dtype=np.int8).astype(dtype)


def real_array(shape, seed, dtype, nonneg=False):
    """Seeded reals with magnitude in [0.5, 2) and random sign (nonneg: all positive), rounded to `dtype`."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 2.0, size=shape)
    if not nonneg:
        a *= rng.choice([-1.0, 1.0], size=shape)
    a = a.astype(dtype)
    mag = np.minimum(np.abs(a), np.nextafter(dtype(2.0), dtype(0.0)))          # rounding to fp32 can reach 2.0 itself
    return np.copysign(mag, a)


def int_product(X, Y):
    """int64 X @ Y of integer-valued float arrays.  Formed by the float64 BLAS product: every partial sum is an integer below 2^53
    (asserted), so that product is exact in any order, and it is far faster than numpy's int64 loop; test_geometry_inputs_cpu.py
    compares it with the int64 loop itself."""
    X64, Y64 = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    assert np.array_equal(X64, np.rint(X64)) and np.array_equal(Y64, np.rint(Y64))
    assert np.abs(X64).max(initial=0) * np.abs(Y64).max(initial=0) * X64.shape[-1] < 2 ** 53
    return (X64 @ Y64).astype(np.int64)


def abs_product(X, Y):
    """(|X| |Y|)_ab in float64: the scale of the entrywise bound and, for integer inputs, the largest possible partial sum."""
    return np.abs(np.asarray(X, np.float64)) @ np.abs(np.asarray(Y, np.float64))


def _matmul_rows(X, Y, threads):
    """X @ Y with the rows of X cut over threads (numpy's longdouble matmul is a plain loop that releases the GIL)."""
    p = X.shape[0]
    if threads <= 1 or p < 2 * threads:
        return X @ Y
    cuts = np.linspace(0, p, threads + 1).astype(int)
    with cf.ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda i: X[cuts[i]:cuts[i + 1]] @ Y, range(threads)))
    return np.concatenate(parts, axis=0)


def hi_product(X, Y, dtype, threads=8):
    """X @ Y in the reference precision of `dtype` (float64 for fp32: BLAS; np.longdouble for fp64)."""
    t = hi_type(dtype)
    if t is np.float64:
        return np.asarray(X, t) @ np.asarray(Y, t)
    return _matmul_rows(np.ascontiguousarray(X, dtype=t), np.ascontiguousarray(Y, dtype=t), threads)


def product_bound(X, Y, dtype, partials):
    """Entrywise bound on |fl(X @ Y) - hi_product(X, Y)| for a product reduced in `dtype` in any order, `partials` partial sums."""
    n = X.shape[-1] + partials + 4
    return (gamma(n, U[dtype]) + gamma(n, unit_roundoff(hi_type(dtype)))) * abs_product(X, Y)


def check_real(got, ref_hi, bound):
    """max error / bound (information) after asserting the entrywise bound."""
    err = np.abs(np.asarray(got, ref_hi.dtype) - ref_hi).astype(np.float64)
    ratio = float((err / bound).max()) if err.size else 0.0
    bad = np.argwhere(err > bound)
    assert bad.size == 0, "entrywise bound exceeded at %s: error / bound = %.3g" % (bad[0].tolist(), ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------- dense rhs shapes
# (k, m, n); each reaches, for the dtype x direction pairs named in tests/test_gpu_dense_matrix.py, rows of the table there.
DENSE_SHAPES = [
    (64, 32, 16), (17, 37, 53), (33, 40003, 53), (64, 70004, 36), (96, 53, 40003), (100, 100, 131077), (16, 131077, 100),
    (16, 523780, 37), (128, 200, 300),
]
DENSE_KC = {0: 32, 1: 16}          # reduction indices per chunk: forward, backward
DENSE_F32_ONLY = {(16, 523780, 37)}          # there for the fp32 backward kernel's single slice (m > 1023 x 512); fp64 has it at (16, 131077, 100)
DENSE_CLASSES = {
    "one_slice_one_chunk": "direct write into B, no reduce kernel",
    "one_slice_loop_ragged": "one slice, >= 3 chunks, ragged last chunk: double-buffered loop, several flips, tail, no reduce",
    "slices_one_chunk": "many slices, 1 chunk each",
    "slices_two_chunks": "many slices, exactly 2 chunks: one prefetch and one flip",
    "slices_loop_short_last": "many slices, >= 3 chunks, short last slice: steady state plus ragged end",
    "scalar_loads": "m % 4 != 0 (fp32), odd m (fp64): scalar-load path throughout",
    "mixed_loads": "aligned m, vector and scalar loads mixed in one wave",
}
# what each shape is there for, per dtype x direction ("f32 fwd", ...): asserted through rcppml_hip_rhs_dense_geometry
DENSE_EXPECT = {
    (64, 32, 16): {p: {"one_slice_one_chunk"} for p in ("f32 fwd", "f32 bwd", "f64 fwd", "f64 bwd")},
    (17, 37, 53): {p: {"slices_one_chunk", "scalar_loads"} for p in ("f32 fwd", "f32 bwd", "f64 fwd", "f64 bwd")},
    (33, 40003, 53): {"f32 fwd": {"slices_two_chunks", "scalar_loads"}, "f64 fwd": {"slices_two_chunks", "scalar_loads"},
                      "f32 bwd": {"slices_one_chunk", "scalar_loads"}, "f64 bwd": {"slices_one_chunk", "scalar_loads"}},
    (64, 70004, 36): {"f32 fwd": {"slices_loop_short_last", "mixed_loads"}, "f64 fwd": {"slices_loop_short_last", "mixed_loads"},
                      "f32 bwd": {"slices_one_chunk", "mixed_loads"}, "f64 bwd": {"slices_two_chunks", "mixed_loads"}},
    (96, 53, 40003): {"f32 fwd": {"slices_one_chunk", "scalar_loads"}, "f64 fwd": {"slices_one_chunk", "scalar_loads"},
                      "f32 bwd": {"slices_loop_short_last", "scalar_loads"}, "f64 bwd": {"slices_loop_short_last", "scalar_loads"}},
    (100, 100, 131077): {"f32 fwd": {"one_slice_loop_ragged", "mixed_loads"}, "f64 fwd": {"one_slice_loop_ragged", "mixed_loads"},
                         "f32 bwd": {"slices_loop_short_last", "mixed_loads"}, "f64 bwd": {"slices_loop_short_last", "mixed_loads"}},
    (16, 131077, 100): {"f32 fwd": {"slices_loop_short_last", "scalar_loads"}, "f64 fwd": {"slices_loop_short_last", "scalar_loads"},
                        "f32 bwd": {"slices_two_chunks", "scalar_loads"}, "f64 bwd": {"one_slice_loop_ragged", "scalar_loads"}},
    (16, 523780, 37): {"f32 fwd": {"slices_loop_short_last", "mixed_loads"}, "f32 bwd": {"one_slice_loop_ragged", "mixed_loads"}},
    (128, 200, 300): {p: {"slices_one_chunk"} for p in ("f32 fwd", "f32 bwd", "f64 fwd", "f64 bwd")},
}
DENSE_MISALIGNED = (128, 200, 300)          # also run with A's base pointer one element off a 16-byte boundary
DENSE_ROW_TILES = {np.float32: {1, 2, 3, 4}, np.float64: {1, 2, 4, 8}}


def dense_pair(dtype, transposed):
    return ("f32" if dtype == np.float32 else "f64") + (" bwd" if transposed else " fwd")


def dense_classes(geom, dtype, m, n, transposed):
    """The rows of the table a launch reaches, from the geometry query's answer (blocks, slices, rows_per_slice, row_tiles)."""
    red, kc = (n, DENSE_KC[1]) if transposed else (m, DENSE_KC[0])
    slices, per = geom["slices"], geom["rows_per_slice"]
    assert per % kc == 0 and (slices - 1) * per < red <= slices * per
    full = per // kc
    last = red - (slices - 1) * per
    last_chunks = -(-last // kc)
    c = set()
    if slices == 1 and last_chunks == 1:
        c.add("one_slice_one_chunk")
    if slices == 1 and last_chunks >= 3 and red % kc:
        c.add("one_slice_loop_ragged")
    if slices > 1 and full == 1:
        c.add("slices_one_chunk")
    if slices > 1 and full == 2:
        c.add("slices_two_chunks")
    if slices > 1 and full >= 3 and last < per:
        c.add("slices_loop_short_last")
    f32 = dtype == np.float32
    if m % (4 if f32 else 2):
        c.add("scalar_loads")
    elif not transposed and m % (16 if f32 else 8):          # a lane's 16 (8) rows of the last chunk run past row m: that lane loads scalars
        c.add("mixed_loads")
    elif transposed and m % (128 if f32 else 32):            # the last wave's lanes past row m take the guarded scalar branch
        c.add("mixed_loads")
    return c


# ---------------------------------------------------------------------------------------------------------------- reduction sizes
def odd_beyond(threshold):
    """An odd size 10 % beyond a threshold."""
    return (int(threshold * 1.1) + 1) | 1


def gram_nblk(dtype, r, cus):
    """Blocks of partial tiles (gram_launch.hip.h); gram_finalize's 32 lanes stride over them."""
    step = 2 if dtype == np.float32 else 4
    return max(1, min((r // step + 127) // 128, 2 * cus))


def gram_cap_r(dtype, cus):
    """Smallest r at which the Gram's block count reaches its cap 2 * CUs."""
    return 2 * cus * 128 * (2 if dtype == np.float32 else 4)


def gram_hi_and_bound(F, eps, cus):
    """F^T F + eps I in the reference precision and the entrywise bound gamma_n sqrt(G_aa G_bb) + eps I, n = r + 4 nblk (one partial
    sum per wave) + 4; sqrt(G_aa G_bb) >= (|F|^T |F|)_ab by Cauchy-Schwarz.  F: (r, k) array = column-major k x r."""
    dtype = F.dtype.type
    r, k = F.shape
    G_hi = hi_product(np.ascontiguousarray(F.T), F, dtype)
    dg = np.diag(G_hi).astype(np.float64)
    n = r + 4 * gram_nblk(dtype, r, cus) + 4
    g = gamma(n, U[dtype]) + gamma(n, unit_roundoff(hi_type(dtype)))
    return G_hi + eps * np.eye(k, dtype=G_hi.dtype), g * np.sqrt(np.outer(dg, dg)) + eps * np.eye(k)


def gram_cases(cus=CUS_DEFAULT):
    """(dtype, k, r, misaligned)"""
    f32, f64 = np.float32, np.float64
    cases = [(dt, k, r, False) for dt in (f32, f64) for k, r in ((5, 1), (16, 2), (33, 3), (64, 5))]
    cases += [(f32, 64, 20003, False), (f32, 33, 20003, False), (f32, 97, 20003, False), (f32, 100, 20003, False), (f64, 48, 20003, False)]
    cases += [(f32, k, odd_beyond(gram_cap_r(f32, cus)), False) for k in (16, 64)]
    cases += [(f64, k, odd_beyond(gram_cap_r(f64, cus)) + 2, False) for k in (16, 32)]
    cases += [(f32, 64, 20003, True)]
    return cases


def row_norm_cases(cus=CUS_DEFAULT):
    """(dtype, k, ncols): second trip of row_norm_final (more than 64 blocks of 256 columns), and both caps -- 2 CUs blocks of
    row_norms (256 columns each) and 8 CUs blocks of apply_scaling (256 threads, one element or one 16-byte vector each)."""
    out = []
    for dt, ks in ((np.float32, (64, 10)), (np.float64, (32, 7))):
        vec = 4 if dt == np.float32 else 2
        for k in ks:
            per_thread = vec if k % vec == 0 else 1
            cap = max(2 * cus * 256, -(-8 * cus * 256 * per_thread // k))
            out += [(dt, k, 16385 + 12), (dt, k, odd_beyond(cap))]
    return out


def sumsq_lengths(cus=CUS_DEFAULT):
    """Second trip of the single-block final pass (more than 256 partials of 2048 elements) and the 4 CUs block cap."""
    return [524288 + 77, odd_beyond(4 * cus * 2048)]


def elementwise_length(cus=CUS_DEFAULT):
    """10 % beyond the 8 CUs x 256 threads cap of mul_rows, axpy and clip_upper."""
    return odd_beyond(8 * cus * 256)
