"""Dense right-hand sides (rcppml_hip_rhs_dense: the four MFMA kernels of kernels_dense.hip.h and dense_reduce) at every launch
geometry the host rule of ops_dense.hip can pick, against a plain high-precision product.

The host code cuts the reduction into chunks (32 indices forward, 16 backward) and slices of whole chunks; the kernels run a
double-buffered loop over a slice's chunks (prefetch the next chunk, park it in the other LDS buffer, copy a = an, flip) and either
write B directly (one slice) or leave per-slice partials to dense_reduce.  Every case asserts through
rcppml_hip_rhs_dense_geometry that it reaches the class of the table it is there for, so a later change of the host rule fails
here instead of quietly losing coverage (tests/geometry_inputs.py: DENSE_CLASSES, DENSE_EXPECT;
tests/test_geometry_inputs_cpu.py asserts on the CPU that every dtype x direction reaches every class and every row-tile variant).

Two legs per case (tests/geometry_inputs.py): integer data, bitwise against the int64 product -- one dropped, doubled or misplaced
term fails it at any size -- and real data within the entrywise bound gamma_n (|A|^T |F|), n = reduction + slices + 4.  Each product
runs twice into outputs pre-filled with different values and must give the same bits: B and the slice partials are fully
overwritten.

Largest observed error / bound of the real leg (information, not asserted): fp32 forward 0.045, fp32 backward 0.11,
fp64 forward 0.060, fp64 backward 0.091, all at the shortest reductions (16 to 53 terms); 1e-5 to 1e-7 at reductions of 40003 terms
and more, where the rounding errors average out and the worst-case bound does not (MI355X)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import geometry_inputs as gi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0)


def _run(torch, _abi, ctx, dtype, dA, m, n, transposed, F, k):
    """The product into two differently pre-filled outputs; asserts they agree bitwise, returns one."""
    dt = _abi.F32 if dtype == np.float32 else _abi.F64
    dF = torch.from_numpy(F).cuda()
    out_cols = m if transposed else n
    outs = []
    for fill in (-7.0, float("nan")):
        dB = torch.full((out_cols, k), fill, dtype=dF.dtype, device="cuda")
        ctx.rhs_dense(dt, dA, m, n, transposed, dF, k, dB)
        outs.append(dB.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "result depends on what the output (or the slice partials) held before"
    return outs[0]


def _both_legs(env, dtype, k, m, n, misaligned=False):
    torch, _abi, ctx = env
    dt = _abi.F32 if dtype == np.float32 else _abi.F64
    ratios = {}
    for leg, make in (("int", gi.int_array), ("real", gi.real_array)):
        At = make((n, m), 1000 * k + m + n, dtype)                       # At[j, i] = A[i, j]: memory = column-major m x n
        if misaligned:
            buf = torch.empty(m * n + 4, dtype=torch.from_numpy(At).dtype, device="cuda")
            assert buf.data_ptr() % 16 == 0
            dA = buf[1:1 + m * n]
            dA.copy_(torch.from_numpy(At).reshape(-1))
            assert dA.data_ptr() % 16 == At.itemsize
        else:
            dA = torch.from_numpy(At).cuda()
            assert dA.data_ptr() % 16 == 0
        for transposed in (0, 1):
            geom = _abi.Context.rhs_dense_geometry(dt, m, n, k, transposed)
            want = gi.DENSE_EXPECT[(k, m, n)][gi.dense_pair(dtype, transposed)]
            assert want <= gi.dense_classes(geom, dtype, m, n, transposed), (geom, want)
            rows = n if transposed else m
            F = make((rows, k), 77 + k + rows + transposed, dtype)
            X = At.T if transposed else At                               # B (out_cols x k) = X @ F
            B = _run(torch, _abi, ctx, dtype, dA, m, n, transposed, F, k)
            if leg == "int":
                assert gi.abs_product(X, F).max() < gi.INT_EXACT_LIMIT
                assert np.array_equal(B.astype(np.int64), gi.int_product(X, F)) and np.array_equal(B, np.rint(B)), (geom, transposed)
            else:
                ratios[transposed] = gi.check_real(B, gi.hi_product(X, F, dtype), gi.product_bound(X, F, dtype, geom["slices"]))
    print("rhs_dense %s k=%d m=%d n=%d%s: error/bound fwd %.2e bwd %.2e" % (np.dtype(dtype).name, k, m, n, " misaligned" if misaligned else "",
                                                                           ratios[0], ratios[1]))


CASES = [(dt, s) for s in gi.DENSE_SHAPES for dt in (np.float32, np.float64) if not (dt == np.float64 and s in gi.DENSE_F32_ONLY)]


@pytest.mark.parametrize("dtype,shape", CASES, ids=["%s-k%d-m%d-n%d" % ((np.dtype(d).name,) + s) for d, s in CASES])
def test_rhs_dense_geometry_class(env, dtype, shape):
    _both_legs(env, dtype, *shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rhs_dense_misaligned_base(env, dtype):
    """m is a multiple of the vector width but A starts one element off a 16-byte boundary: the kernels must take their scalar
    loads (a 16-byte load of such an address is not the same bytes)."""
    _both_legs(env, dtype, *gi.DENSE_MISALIGNED, misaligned=True)


def test_dense_fit_where_the_loop_iterates():
    """One whole fit through the dense fp64 plugin entry at 40003 x 53 (forward: 626 slices of two chunks; backward: 4 slices),
    against the oracle's unfused fit, at the bars of test_gpu_dense.py::test_dense_fit_through_plugin."""
    from rcppml_amd import _abi
    m, n, k = 40003, 53, 6
    rng = np.random.default_rng(3)
    M = rng.uniform(0, 1, (m, 4)) @ rng.uniform(0, 1, (4, n)) + 0.05 * rng.standard_normal((m, n))
    M = np.maximum(M, 0.0)
    M[rng.random((m, n)) < 0.3] = 0.0
    geom = _abi.Context.rhs_dense_geometry(_abi.F64, m, n, k, 0)
    assert geom["slices"] > 1 and geom["rows_per_slice"] >= 2 * gi.DENSE_KC[0]
    W0, H0 = O.init_factors(9, k, m, n, np.float64)
    ref = O.nmf_fit(O.dense_as_csc(M), W0, H0, np.float64, max_iter=3, tol=0.0, solver_mode=0, unfused=True, sort_model=True)
    W, H = W0.copy(), H0.copy()
    res = _abi.nmf_dense(M, k, W, H, entry="double", max_iter=3, tol=0.0, solver_mode=0)
    assert res["status"] == 0, res["error"]
    assert res["iter"] == ref.iter
    assert abs(res["loss"] - ref.loss) / abs(ref.loss) < 1e-6
    assert np.abs(res["d"] - ref.d).max() / np.abs(ref.d).max() < 1e-6
    assert np.abs(W - ref.W_T).max() < 1e-6 and np.abs(H - ref.H).max() < 1e-6
