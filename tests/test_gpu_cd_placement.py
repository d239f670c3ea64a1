"""The explicitly placed launches of the MFMA CD solves (cd_mfma_placed_kernel, 32-column tiles; cd_mfma64_placed_kernel,
16-column tiles: one workgroup per CU, static tile map of rcppml_amd/csrc/cd_placement.hip.h) against the launches they replace
(cd_mfma_kernel / cd_mfma64_kernel, one workgroup per four tiles), bit for bit on the solutions and on the per-column sweep
counts.  Both forms run every tile through the same body; the reference forms are themselves pinned to float64 by the
committed CD tests.

The launch is told to assume 2 CUs (RCPPML_OPT_CD_ASSUME_CUS: 8 SIMDs), so that a few hundred columns reach every branch of
the map:
  805 columns  = 25 tiles + a 5-column one on 8 SIMDs: three rounds (up, down, down), two left-over tiles, a partial tile;
  4133 columns = 130 tiles: four rounds, 98 left-over tiles (last-round waves loop over several), and a work order long
                 enough for the serpentine layout of rcppml_hip_order_columns to reverse a group, which the kernel undoes;
  1, 31, 33, 256 columns: fewer tiles than SIMDs -- forced (RCPPML_OPT_CD_PLACED = 1) most waves have no tile; left to the
                 selection (= 0) these sizes keep the old launch.
16-column tiles (selected between one and two tiles per SIMD, two rounds of waves):
  197 columns  = 12 tiles + a 5-column one: the second round holds the five surplus tiles, the other second-round waves none;
  805, 4133 columns (forced): 51 and 259 tiles, second-round waves loop over left-over tiles; 4133 also reverses a group."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [805, 4133, 197, 1, 31, 33, 256]


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    ctx = _abi.Context(0)
    return torch, _abi, ctx


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_PROBLEMS = {}


def _problem(n, k):
    """Gram, right-hand sides, a non-negative warm start and two work orders (a random permutation; the layout
    rcppml_hip_order_columns makes of random sweep counts), formed once per (n, k) and left unchanged."""
    if (n, k) not in _PROBLEMS:
        rs = np.random.default_rng(1000 * k + n)
        Fm = rs.uniform(size=(4 * k, k))
        G = (Fm.T @ Fm).astype(np.float32)
        B = (rs.standard_normal((n, k)) * 2 + 1).astype(np.float32)
        X0 = np.maximum(rs.standard_normal((n, k)), 0).astype(np.float32)
        perm = rs.permutation(n).astype(np.int32)
        sw = rs.integers(0, 100, size=n).astype(np.int32)
        _PROBLEMS[(n, k)] = (G, B, X0, perm, sw)
    return _PROBLEMS[(n, k)]


def _solve(env, mode, variant, n, k, G, B, X0, warm, order, maxit, tol):
    torch, _abi, ctx = env
    dX = _dev(torch, X0) if warm else torch.full((n, k), 7.0, dtype=torch.float32, device="cuda")
    d_sw = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ctx.set_option(_abi.OPT_CD_ASSUME_CUS, 2)
    ctx.set_option(_abi.OPT_CD_PLACED, mode)
    try:
        ctx.solve_cd(_abi.F32, G, B, dX, k, n, warm=int(warm), zero_init=int(not warm), maxit=maxit, tol=tol, variant=variant,
                     sweeps_out=d_sw, col_order=order)
        ctx.sync()
    finally:
        ctx.set_option(_abi.OPT_CD_PLACED, 0)
        ctx.set_option(_abi.OPT_CD_ASSUME_CUS, 0)
    return dX.cpu().numpy(), d_sw.cpu().numpy()


@pytest.mark.parametrize("order_kind", ["none", "perm", "sorted"])
@pytest.mark.parametrize("warm", [True, False])
@pytest.mark.parametrize("k", [17, 64])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("tile", [32, 16])
def test_placed_launch_matches_tile_per_wave_launch(env, tile, n, k, warm, order_kind):
    torch, _abi, ctx = env
    variant = _abi.CD_MFMA if tile == 32 else _abi.CD_MFMA16
    G, B, X0, perm, sw = _problem(n, k)
    dG, dB = _dev(torch, G), _dev(torch, B)
    order = None
    if order_kind == "perm":
        order = _dev(torch, perm)
    elif order_kind == "sorted":
        order = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ctx.order_columns(_dev(torch, sw), n, order)
    for maxit in (7, 100):
        for tol in (0.0, 1e-8):
            ref_x, ref_sw = _solve(env, 2, variant, n, k, dG, dB, X0, warm, order, maxit, tol)
            assert ref_sw.min() >= 1 and ref_sw.max() <= maxit            # every column was solved by the reference form
            for mode in (1, 0):                                           # forced; chosen by tiles per SIMD
                x, s = _solve(env, mode, variant, n, k, dG, dB, X0, warm, order, maxit, tol)
                assert np.array_equal(s, ref_sw), (mode, maxit, tol)
                assert np.array_equal(x.view(np.uint32), ref_x.view(np.uint32)), (mode, maxit, tol)
