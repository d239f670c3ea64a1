"""Gram and the O(k n) reductions at the launch geometries their host code picks from the problem size: the second trip of the
final passes that stride over block partials (gram_finalize b += 32, row_norm_final b += 64, sum_partials / loss_mse_final
i += 256) and the block-count caps (2 CUs: Gram, row_norms; 4 CUs: sumsq, loss_mse; 8 CUs: apply_scaling, mul_rows, axpy,
clip_upper), each 10 % beyond its threshold at an odd size.  The CU count comes from the device; the thresholds from the rules
next to the launches (tests/geometry_inputs.py restates them, tests/test_geometry_inputs_cpu.py checks the sizes cross them).

Integer data (tests/geometry_inputs.py) makes every sum exact in fp32 and fp64 in any order: the comparison is bitwise, and one
dropped or doubled block partial fails it.  The Gram also gets the real-valued leg: entrywise within gamma_n (|F|^T |F|)_ab,
n = r + 4 nblk (one partial per wave) + 4, against float64 (fp32) / longdouble (fp64).

Largest observed error / bound of the Gram's real leg (information, not asserted): fp32 0.16, fp64 0.13 (both at r = 5), 1.2e-4 at
r = 20003, 1.1e-5 (fp32) and 3.7e-6 (fp64) beyond the block cap (MI355X)."""
import numpy as np
import pytest

from tests import geometry_inputs as gi

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0), torch.cuda.get_device_properties(0).multi_processor_count


def _dt(_abi, dtype):
    return _abi.F32 if dtype == F32 else _abi.F64


def _dev(torch, a, misaligned=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not misaligned:
        return t.cuda()
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def _case_id(c):
    return "%s-k%d-r%d%s" % (np.dtype(c[0]).name, c[1], c[2], "-misaligned" if c[3] else "")


# the case list is built for the MI355X's 256 CUs so that test ids are stable; the test recomputes the sizes from the device's count
@pytest.mark.parametrize("index", range(len(gi.gram_cases())), ids=[_case_id(c) for c in gi.gram_cases()])
def test_gram_geometry(env, index):
    torch, _abi, ctx, cus = env
    dtype, k, r, misaligned = gi.gram_cases(cus)[index]
    nblk = gi.gram_nblk(dtype, r, cus)
    if r == 20003:
        assert 32 < nblk < 2 * cus          # gram_finalize's lanes take a second trip, below the cap
    elif r > 20003:
        assert nblk == 2 * cus and r > 1.1 * gi.gram_cap_r(dtype, cus)
    ratio = 0.0
    for leg, make in (("int", gi.int_array), ("real", gi.real_array)):
        F = make((r, k), k + r, dtype)          # (r, k) array = column-major k x r
        dG = torch.full((k, k), float("nan"), dtype=torch.from_numpy(F).dtype, device="cuda")
        ctx.gram(_dt(_abi, dtype), _dev(torch, F, misaligned), k, r, 0.0, 0.0, dG)
        G = dG.cpu().numpy()
        assert np.array_equal(G, G.T), "Gram must be bitwise symmetric"
        Ft = np.ascontiguousarray(F.T)
        if leg == "int":
            assert gi.abs_product(Ft, F).max() < gi.INT_EXACT_LIMIT
            assert np.array_equal(G, np.rint(G)) and np.array_equal(G.astype(np.int64), gi.int_product(Ft, F))
        else:
            ratio = gi.check_real(G, gi.hi_product(Ft, F, dtype), gi.product_bound(Ft, F, dtype, 4 * nblk))
    print("gram %s k=%d r=%d nblk=%d: error/bound %.2e" % (np.dtype(dtype).name, k, r, nblk, ratio))


@pytest.mark.parametrize("norm_type", [0, 1, 2])
@pytest.mark.parametrize("index", range(len(gi.row_norm_cases())), ids=["%s-k%d-c%d" % (np.dtype(c[0]).name, c[1], c[2]) for c in gi.row_norm_cases()])
def test_row_norms_and_scaling_geometry(env, index, norm_type):
    """row_norms: integer entries in {0..3}, so the sums of |x| (norm_type 0) and of x^2 (1, 2) are exact: bitwise.
    apply_scaling (scale_rows_from_sums / _vec: s = sums[f]; norm_type 1: s = sqrt(s); d = s + 1e-15; X = X / d), in units of
    the unit roundoff u:
      norm_type 0: s is the exact integer sum, >= 16, where 1e-15 is below half a unit in the last place of fp32 and fp64 (asserted
        on the host), so d = s exactly; the quotient is one division (<= 1 u) or, should the compiler form it that way, a
        reciprocal (<= 2 u) and a product (<= 1 u): <= 3 u relative, which is below 3 units in the last place of the result.
      norm_type 1: the square root adds <= 2 u (1 unit in the last place) to d, so d is within 1 unit in the last place of the
        exact root and the scaled entries within 5.
      norm_type 2: d = 1 and X is not touched: bitwise."""
    torch, _abi, ctx, cus = env
    dtype, k, c = gi.row_norm_cases(cus)[index]
    dt = _dt(_abi, dtype)
    hi = gi.hi_type(dtype)
    nblk = min(-(-c // 256), 2 * cus)
    assert nblk > 64          # row_norm_final's 64 lanes take a second trip
    X = gi.int_array((c, k), k + c, dtype, nonneg=True)
    S = (np.abs(X) if norm_type == 0 else X * X).astype(np.int64).sum(axis=0)
    assert S.min() >= 16 and S.max() < gi.INT_EXACT_LIMIT
    dX = _dev(torch, X)
    sums = torch.full((k,), float("nan"), dtype=dX.dtype, device="cuda")
    d = torch.full((k,), float("nan"), dtype=dX.dtype, device="cuda")
    ctx.row_norms(dt, dX, k, c, norm_type, sums)
    assert np.array_equal(sums.cpu().numpy().astype(np.int64), S) and sums.dtype == dX.dtype
    ctx.apply_scaling(dt, dX, k, c, norm_type, sums, d)
    dg, Xg = d.cpu().numpy(), dX.cpu().numpy()
    if norm_type == 2:
        assert np.array_equal(dg, np.ones(k, dtype)) and np.array_equal(Xg, X)
        return
    d_hi = S.astype(hi) if norm_type == 0 else np.sqrt(S.astype(hi))
    if norm_type == 0:
        assert np.array_equal(S.astype(dtype) + dtype(1e-15), S.astype(dtype))          # the + 1e-15 vanishes at these magnitudes
        assert np.array_equal(dg.astype(np.int64), S) and np.array_equal(dg, np.rint(dg))
    else:
        assert np.all(np.abs(dg.astype(hi) - d_hi) <= np.spacing(d_hi.astype(dtype)).astype(hi))
    X_hi = X.astype(hi) / d_hi[None, :]
    ulps = 3 if norm_type == 0 else 5
    err = np.abs(Xg.astype(hi) - X_hi)
    assert np.all(err <= ulps * np.spacing(np.abs(X_hi).astype(dtype)).astype(hi)), float((err / np.spacing(np.abs(X_hi).astype(dtype) + np.finfo(dtype).tiny)).max())


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("which", [0, 1], ids=["final-second-trip", "beyond-cap"])
def test_sumsq_and_loss_mse_geometry(env, dtype, which):
    """sumsq and the three outputs of loss_mse accumulate in double: with integer x, d, W_T, B_w and Gram inputs they are exact."""
    torch, _abi, ctx, cus = env
    dt = _dt(_abi, dtype)
    length = gi.sumsq_lengths(cus)[which]
    nblk = min(-(-length // 2048), 4 * cus)
    assert nblk > 256 and (which == 0 or -(-length // 2048) > 4 * cus)
    x = gi.int_array((length,), length, dtype)
    out1 = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.sumsq(dt, _dev(torch, x), length, out1)
    tr_ref = int((x.astype(np.int64) ** 2).sum())
    assert out1.item() == tr_ref
    k = 5 if which == 0 else 7
    m = -(-length // k)          # k m >= length: the same number of blocks or more
    assert min(-(-k * m // 2048), 4 * cus) >= nblk
    W = gi.int_array((m, k), 11 + m, dtype)
    Bw = gi.int_array((m, k), 12 + m, dtype)
    d = gi.int_array((k,), 13, dtype, nonneg=True) + dtype(1)
    Gw, Gs = gi.int_array((k, k), 14, dtype), gi.int_array((k, k), 15, dtype)
    i64 = lambda a: a.astype(np.int64)
    cross = int((i64(d)[None, :] * i64(W) * i64(Bw)).sum())
    recon = int((np.outer(i64(d), i64(d)) * i64(Gw) * i64(Gs)).sum())
    out = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    ctx.loss_mse(dt, out1, _dev(torch, d), _dev(torch, W), _dev(torch, Bw), k, m, _dev(torch, Gw), _dev(torch, Gs), out)
    o = out.cpu().numpy()
    assert abs(cross) > 0 and (o[1], o[2], o[0]) == (cross, recon, tr_ref - 2 * cross + recon)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_elementwise_ops_beyond_the_block_cap(env, dtype):
    """mul_rows, axpy and clip_upper launch at most 8 CUs blocks of 256 threads and stride: 10 % more elements than that,
    integer data, exact."""
    torch, _abi, ctx, cus = env
    dt = _dt(_abi, dtype)
    k = 7
    c = -(-gi.elementwise_length(cus) // k)
    n = k * c
    assert -(-n // 256) > 8 * cus
    X = gi.int_array((c, k), 21, dtype)
    T = gi.int_array((c, k), 22, dtype)
    d = gi.int_array((k,), 23, dtype, nonneg=True) + dtype(1)
    dX, dT = _dev(torch, X), _dev(torch, T)
    dY = torch.full((c, k), float("nan"), dtype=dX.dtype, device="cuda")
    ctx.mul_rows(dt, dX, k, c, _dev(torch, d), dY)
    assert np.array_equal(dY.cpu().numpy(), X * d[None, :])
    dY.fill_(float("nan"))
    ctx.axpy(dt, dX, dT, 3.0, n, dY)
    assert np.array_equal(dY.cpu().numpy(), X + dtype(3) * T)
    ctx.clip_upper(dt, dX, n, 1.0)
    assert np.array_equal(dX.cpu().numpy(), np.minimum(X, dtype(1)))
