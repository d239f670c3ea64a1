"""Wave priorities in the fp32 MFMA CD solves (RCPPML_OPT_CD_PRIO; kernels_cd_mfma.hip.h, kernels_cd_mfma64.hip.h) must not
change a bit: s_setprio only decides which ready wave of a SIMD issues next.  Every mode the selector accepts (1, 2 static by
round, 3, 4 dynamic) is held to mode 0 on the solutions and on the per-column sweep counts, with torch.equal, with and without
a sweep-sorted work order, on early-exit solves (warm start, at most 100 sweeps, tol 1e-8, non-negative).

The explicitly placed launches are forced (RCPPML_OPT_CD_PLACED = 1) and told to assume 4 CUs = 16 SIMDs, so that the smallest
sizes reach the rounds the static modes tell apart:
  32-column tiles, 1573 columns = 49 tiles + a 5-column one: three rounds of waves, two left-over tiles, a partial last tile;
  32-column tiles, 2100 columns = 65 tiles + a 20-column one: four rounds (priorities 0..3), two left-over tiles;
  16-column tiles,  389 columns = 24 tiles + a 5-column one: a second round of 9 surplus waves beside 7 empty ones.
Each at k = 64, k = 40 (padded to 64 / 48) and k = 24 (one 32-row tile / two 16-row tiles).  The tile-per-wave launches
(RCPPML_OPT_CD_PLACED = 2) run at 200 and 70 columns: there the dynamic modes have kernels of their own and the static ones fall
back to mode 0.  The inputs (tests/cd_prio_inputs.py) spread the sweep counts from 1 to the cap, so frozen columns, the early
exit of a whole tile and the cap are all met; the spread is asserted on the mode-0 counts."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import cd_prio_inputs as pi
from tests.cd_inputs import cd_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    ctx = _abi.Context(0)
    return torch, _abi, ctx


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _solve(env, tile, placed, prio, n, k, dG, dB, X0, order, **kw):
    """One solve on the `tile`-column form with priority mode `prio` on that form's side of the option (None: the context's
    default, untouched).  Returns the device tensors (X, sweeps)."""
    torch, _abi, ctx = env
    dX = _dev(torch, X0) if X0 is not None else torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    d_sw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.set_option(_abi.OPT_CD_ASSUME_CUS, 4)
    ctx.set_option(_abi.OPT_CD_PLACED, placed)
    if prio is not None:
        ctx.set_option(_abi.OPT_CD_PRIO, _abi.cd_prio_value(prio, 0) if tile == 32 else _abi.cd_prio_value(0, prio))
    try:
        ctx.solve_cd(_abi.F32, dG, dB, dX, k, n, variant=_abi.CD_MFMA if tile == 32 else _abi.CD_MFMA16, sweeps_out=d_sw,
                     col_order=order, **kw)
        ctx.sync()
    finally:
        ctx.set_option(_abi.OPT_CD_PRIO, _abi.CD_PRIO_DEFAULT)
        ctx.set_option(_abi.OPT_CD_PLACED, 0)
        ctx.set_option(_abi.OPT_CD_ASSUME_CUS, 0)
    return dX, d_sw


def _check_modes(env, tile, placed, n, k):
    torch, _abi, ctx = env
    G, B, X0 = pi.problem(n, k)
    dG, dB = _dev(torch, G), _dev(torch, B)
    kw = dict(warm=1, maxit=pi.MAXIT, tol=pi.TOL)
    ref_x, ref_sw = _solve(env, tile, placed, 0, n, k, dG, dB, X0, None, **kw)
    sw = ref_sw.cpu().numpy()
    print("tile %d placed %d n %d k %d: mode-0 sweeps min %d median %d max %d" % (tile, placed, n, k, sw.min(), np.median(sw), sw.max()))
    assert sw.min() >= 1 and sw.min() <= 5 and sw.max() == pi.MAXIT            # a handful ... the cap
    order = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.order_columns(ref_sw, n, order)                                        # longest first, as a fit orders its next solve
    for od in (None, order):
        for mode in _abi.CD_PRIO_MODES:
            if mode == 0 and od is None:
                continue
            x, s = _solve(env, tile, placed, mode, n, k, dG, dB, X0, od, **kw)
            assert torch.equal(s, ref_sw), (mode, od is not None)
            assert torch.equal(x, ref_x), (mode, od is not None)


@pytest.mark.parametrize("k", pi.KS)
@pytest.mark.parametrize("tile,n", pi.PLACED_SHAPES)
def test_priorities_change_no_bit_placed(env, tile, n, k):
    _check_modes(env, tile, 1, n, k)


@pytest.mark.parametrize("k", pi.KS)
@pytest.mark.parametrize("n", pi.TILE_PER_WAVE_NS)
@pytest.mark.parametrize("tile", [32, 16])
def test_priorities_change_no_bit_tile_per_wave(env, tile, n, k):
    _check_modes(env, tile, 2, n, k)


@pytest.mark.parametrize("tile,n", [(32, 1573), (16, 389)])
def test_mode0_and_default_against_float64_oracle(env, tile, n):
    """Mode 0 and what a new context runs (RCPPML_CD_PRIO_DEFAULT) against the oracle's nnls_batch in float64: cold start, k = 64,
    the inputs and the bound of tests/test_gpu_kernels.py::test_cd_cold (2e-4 of the largest entry; the float32 oracle itself is
    4e-7 from the float64 one on these inputs)."""
    torch, _abi, ctx = env
    k = 64
    G, B, _ = cd_problem(k, n, np.float32, 900 + n)
    X_ref = O.nnls_batch(G.astype(np.float64), B.astype(np.float64), maxit=100, tol=1e-8)
    dG, dB = _dev(torch, G), _dev(torch, B)
    scale = np.abs(X_ref).max()
    for prio in (0, None):
        dX, _ = _solve(env, tile, 1, prio, n, k, dG, dB, None, None, zero_init=1, maxit=100, tol=1e-8)
        X = dX.cpu().numpy()
        err = np.abs(X - X_ref).max() / scale
        print("tile %d prio %s: max|X - X_ref| / max|X_ref| = %.3g" % (tile, prio, err))
        assert X.min() >= 0
        assert err < 2e-4


def test_out_of_range_value_is_refused_by_the_library(env):
    torch, _abi, ctx = env
    L = _abi.lib()
    for bad in (-1, 5, 7, 8 * 5, 8 * 4 + 5, 64, 1 << 20):
        assert L.rcppml_hip_ctx_set_option(ctx._h, _abi.OPT_CD_PRIO, bad) != 0, bad
        with pytest.raises(_abi.BackendError):
            ctx.set_option(_abi.OPT_CD_PRIO, bad)
    for h in _abi.CD_PRIO_MODES:
        for w in _abi.CD_PRIO_MODES:
            ctx.set_option(_abi.OPT_CD_PRIO, _abi.cd_prio_value(h, w))
    ctx.set_option(_abi.OPT_CD_PRIO, _abi.CD_PRIO_DEFAULT)
