"""rcppml_hip_solve_cd, every kernel it dispatches to, against the float64 restatement tests/cd_ref.py (pinned to the oracle by
tests/test_cd_ref_cpu.py): options at every KP / RT / NT case of the dispatch switch and every LPC a rank selects by itself,
work-order invariance, early exit and per-column sweep counts, the AUTO thresholds, ragged column counts.  X and B carry 64
sentinel rows behind row ncols.

Bounds (relative to max|ref|, the project's existing ones -- cd_inputs.cd_tolerance): fp64 1e-9; fp32 3e-4, x 4 for 64 < k <= 128,
x 16 for k > 128; x 10 without non-negativity.

Conditions on the inputs, measured on the CPU alone (tests/test_cd_ref_cpu.py::test_input_conditions_fp32 asserts them):
  D = deviation of the fp32 ORACLE from the float64 restatement, as a fraction of the fp32 bound, worst option per k, with the
  ridge cd_inputs.OPTION_RIDGE = 0.25 (without it 0.27 at k = 48):
    k      1     9     16    17    32    40    48    64    70    96    100   128   129   256
    D/b  0.001 0.011 0.028 0.029 0.099 0.107 0.173 0.222 0.061 0.121 0.121 0.156 0.045 0.110
  column counts (k = 48 / 100, each run against the columns it solved): D/b <= 0.054 / 0.051 for n >= 15, 0.155 / 0.058 at n = 1
  early exit (ridge cd_inputs.EARLY_RIDGE = 1.0, where the D that asks for it is recorded; seeds cd_inputs.EARLY_SEED, n = 129): share of non-decisive columns (stop statistic within tol (1 +- delta) at some
  sweep; delta 1e-2 fp32, 1e-6 fp64), as (tol 1e-8 cold, warm, tol 1e-3 cold, warm):
    fp32  k = 9: 0.008 0.023 0.000 0.000   k = 32: 0.008 0.023 0.039 0.023   k = 64: 0.023 0.008 0.031 0.008
          k = 128: 0.023 0.031 0.016 0.023                    fp64: 0.000 everywhere
Largest GPU deviation observed on an MI355X, as a fraction of the bound, worst variant and option per k (recorded, never used as
a bound):
    k      1      9     16    17    32    40    48    64    70    96    100   128   129   256
    fp32 0.0007 0.014 0.023 0.029 0.091 0.085 0.140 0.182 0.067 0.135 0.121 0.144 0.046 0.110
    fp64 < 3e-4 of the bound at every k (2.5e-13 absolute at k = 256)
  i.e. the kernels sit where the fp32 oracle sits; every other test of this file stays under 0.19 of its bound.
  test_column_counts, fp32, worst variant: COLCOUNT_GPU
"""
import numpy as np
import pytest

from tests import cd_inputs as I
from tests import cd_ref as R

pytestmark = pytest.mark.gpu

VARIANTS = ["lane", "wave", "group", "mfma", "mfma16", "lmf"]
DTYPES = [np.float32, np.float64]
SENT = 64
SENT_X, SENT_B = -777.25, 555.5


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0)


def _var(_abi, name):
    return dict(lane=_abi.CD_LANE, wave=_abi.CD_WAVE, group=_abi.CD_GROUP, mfma=_abi.CD_MFMA, mfma16=_abi.CD_MFMA16, lmf=_abi.CD_LMF,
                auto=_abi.CD_AUTO)[name]


def _dt(_abi, dtype):
    return _abi.F32 if np.dtype(dtype) == np.float32 else _abi.F64


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Problem:
    """G, B and X0 on the device, X and B padded with sentinel rows; run() solves into a fresh copy of X0 and checks what no
    solve may touch: B and the sentinel rows of X bit for bit."""
    def __init__(self, env, G, B, X0):
        self.torch, self._abi, self.ctx = env
        self.dtype = G.dtype
        self.n, self.k = B.shape
        self.G = _dev(self.torch, G)
        self.Bpad = np.concatenate([B, np.full((SENT, self.k), SENT_B, self.dtype)])
        self.Xpad = np.concatenate([X0, np.full((SENT, self.k), SENT_X, self.dtype)])
        self.B = _dev(self.torch, self.Bpad)

    def run(self, variant, order=None, **kw):
        torch = self.torch
        dX = _dev(torch, self.Xpad)
        sw = torch.full((self.n + SENT,), -5, dtype=torch.int32, device="cuda")
        self.ctx.solve_cd(_dt(self._abi, self.dtype), self.G, self.B, dX, self.k, self.n, variant=_var(self._abi, variant),
                          sweeps_out=sw, col_order=order, **kw)
        X, s = dX.cpu().numpy(), sw.cpu().numpy()
        assert np.array_equal(X[self.n:], self.Xpad[self.n:]), "sentinel rows of X"
        assert np.array_equal(self.B.cpu().numpy(), self.Bpad), "B"
        assert np.all(s[self.n:] == -5), "sweeps_out behind ncols"
        return X[:self.n], s[:self.n]


def _parity(X, Xr, dtype, k, nonneg=True):
    dev = np.abs(X.astype(np.float64) - Xr).max() / np.abs(Xr).max()
    bound = I.cd_tolerance(dtype, k, nonneg)
    print("dev/bound %.3g" % (dev / bound))
    return dev, bound


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", I.OPTION_KS)
def test_options_every_instantiation(env, k, dtype, variant):
    """Fixed 7 sweeps with each of the eleven option sets (cd_inputs.option_cases).  The ranks hit every KP / RT / NT case:
    32-column MFMA RT = 1..4 (k 1..32, 33..64, 65..96, 97..128), 16-column NT = 1..4 (fp32) and 1..8 (fp64: 70 -> 5, 96 -> 6, 100 -> 7,
    128 -> 8), lane KP 16 / 32 / 64 and its GROUP fallback, wave KP 64 / 128, LMF and its AUTO fallback when the step is not the
    plain non-negative one, and the general-rank kernel (129, 256).  Group runs KP 16..128 at the lanes per column pick_lpc gives
    each dtype: (KP, LPC) = (16, 1) (32, 1) (64, 2) (128, 4) in fp32, (16, 1) (32, 2) (64, 4) (128, 4) in fp64.  The other three
    instantiations of the switch, cd_group_kernel<T, 16, 2>, <T, 16, 4> and <T, 32, 4>, are selected only by the experiment variable
    RCPPML_GPU_CD_LPC and run in no test.  Every non-simple option runs the SIMPLE = false bodies."""
    G, B, X0, ub, cases, refs = I.options_reference(dtype, k)
    P = Problem(env, G, B, X0)
    worst = 0.0
    for name, kw in cases.items():
        Xr = refs[name][0]
        X, sw = P.run(variant, **kw)
        nonneg = bool(kw.get("nonneg", 1))
        dev, bound = _parity(X, Xr, dtype, k, nonneg)
        worst = max(worst, dev / bound)
        assert dev < bound, (name, dev, bound)
        if nonneg:
            assert X.min() >= 0, name
        if kw.get("ub_cd", 0) > 0 or kw.get("ub_post", 0) > 0:
            assert X.max() <= dtype(ub), name                   # exactly: the bound is a float32 value
            assert (X == dtype(ub)).any(), name
        assert np.all(sw == 7), (name, sw.min(), sw.max())
    print("worst dev/bound", np.dtype(dtype).name, k, variant, "%.3g" % worst)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [16, 48, 100, 200])
def test_work_order_is_invisible(env, k, dtype, variant):
    """col_order only changes which slot solves which column (include/rcppml_gpu.h: any permutation gives identical results):
    X and sweeps_out bit for bit without an order, with a random permutation and with the reverse order -- early exit on, so
    that a slot's neighbours finish at other sweeps than in the natural order -- with and without non-negativity."""
    torch = env[0]
    n = 257
    G, B, X0 = I.cd_problem(k, n, dtype, 300 + k, ridge=I.EARLY_RIDGE)
    P = Problem(env, G, B, X0)
    perm = np.random.default_rng(k).permutation(n).astype(np.int32)
    orders = [None, _dev(torch, perm), _dev(torch, np.arange(n - 1, -1, -1, dtype=np.int32))]
    for nonneg in (1, 0):
        outs = [P.run(variant, order=o, warm=1, nonneg=nonneg, maxit=25, tol=1e-4) for o in orders]
        for X, sw in outs[1:]:
            assert np.array_equal(X, outs[0][0]), nonneg
            assert np.array_equal(sw, outs[0][1]), nonneg


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", I.EARLY_KS)
def test_early_exit_and_sweep_counts(env, k, dtype, variant):
    """The relative-change stop: iterates, the per-column sweep counts on every decisive column (see the module docstring), and
    the context's work counters against sweeps_out."""
    _, _abi, ctx = env
    delta = I.EARLY_DELTA[np.dtype(dtype)]
    for tol in (1e-8, 1e-3):
        for warm in (False, True):
            G, B, X0, kw, (Xr, swr, stat) = I.early_reference(dtype, k, tol, warm)
            P = Problem(env, G, B, X0)
            ctx.stats(reset=True)
            X, sw = P.run(variant, **kw)
            st = ctx.stats(reset=True)
            dev, bound = _parity(X, Xr, dtype, k)
            assert dev < bound, (tol, warm, dev, bound)
            assert st["cd_columns"] == P.n and st["cd_column_sweeps"] == int(sw.sum()), (tol, warm, st, int(sw.sum()))
            dec = R.decisive(stat, I.q(tol, dtype), delta)
            assert dec.mean() >= 0.95
            bad = np.nonzero(dec & (sw != swr))[0]
            assert bad.size == 0, (tol, warm, bad[:8], sw[bad[:8]], swr[bad[:8]])


def _sampled_check(env, k, dtype, n, seed, nonneg, sample=256):
    """AUTO on n columns; the restatement on `sample` of them (the last column always among them)."""
    G, B, X0 = I.cd_problem(k, n, dtype, seed, ridge=I.EARLY_RIDGE)
    P = Problem(env, G, B, X0)
    tol = 1e-4
    X, sw = P.run("auto", warm=1, nonneg=nonneg, maxit=100, tol=tol)
    idx = np.unique(np.concatenate([np.random.default_rng(seed).choice(n, size=min(sample, n) - 1, replace=False), [n - 1, 0]]))
    Xr, swr, stat = R.cd_solve_batch(G, B[idx], X0[idx], warm=True, nonneg=bool(nonneg), maxit=100, tol=I.q(tol, dtype))
    dev, bound = _parity(X[idx], Xr, dtype, k, bool(nonneg))
    assert dev < bound, (k, n, dev, bound)
    dec = R.decisive(stat, I.q(tol, dtype), I.EARLY_DELTA[np.dtype(dtype)])
    assert dec.mean() >= 0.95
    assert np.array_equal(sw[idx][dec], swr[dec]), (k, n)
    assert sw.min() >= 1 and sw.max() <= 100


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [16, 32, 64])
def test_auto_thresholds_small_side(env, k, dtype):
    """AUTO at ncols = 6 CUs (cd_wave_static_kernel<16 | 32 | 64>) and at 6 CUs + 1 (the 16-column MFMA kernel of either dtype)."""
    cus = env[0].cuda.get_device_properties(0).multi_processor_count
    _sampled_check(env, k, dtype, 6 * cus, 7000 + k, 1)
    _sampled_check(env, k, dtype, 6 * cus + 1, 7100 + k, 1)


def test_auto_thresholds_tile_width(env):
    """fp32, k = 64: 128 CUs - 32 columns are one tile short of 4 CUs tiles of 32 (16-column kernel), 128 CUs columns are not
    (32-column kernel)."""
    cus = env[0].cuda.get_device_properties(0).multi_processor_count
    _sampled_check(env, 64, np.float32, 128 * cus - 32, 7200, 1)
    _sampled_check(env, 64, np.float32, 128 * cus, 7201, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_auto_thresholds_general_step_is_not_static(env, dtype):
    """nonneg = 0 at ncols = 6 CUs: the static kernel only knows the plain non-negative step, AUTO must not take it."""
    cus = env[0].cuda.get_device_properties(0).multi_processor_count
    _sampled_check(env, 32, dtype, 6 * cus, 7300, 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", I.COUNT_KS)
def test_column_counts(env, k, dtype, variant):
    """Column counts around the tile widths (16, 32, 64 columns per wave), warm, 7 fixed sweeps; each run against the columns
    it solved."""
    G, B, X0, Xr = I.count_reference(dtype, k)
    worst = (0.0, 0)
    for n in I.COUNT_NS:
        P = Problem(env, G, B[:n], X0[:n])
        X, sw = P.run(variant, warm=1, maxit=7, tol=0.0)
        dev, bound = _parity(X, Xr[:n], dtype, k)
        worst = max(worst, (dev / bound, n))
        assert dev < bound, (n, dev, bound)
        assert X.min() >= 0 and np.all(sw == 7), n
    print("worst dev/bound", np.dtype(dtype).name, k, variant, "%.3g at n = %d" % worst)
