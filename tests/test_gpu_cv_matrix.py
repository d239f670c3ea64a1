"""rcppml_hip_solve_cv, rcppml_hip_solve_cv_irls, rcppml_hip_cv_test_error and rcppml_hip_cv_irls_loss, every kernel they dispatch
to, against the float64 restatement tests/cv_ref.py (pinned to the oracle by tests/test_cv_ref_cpu.py) on the edge matrix of
tests/cv_inputs.py: every dispatch point x every option case x both mask_zeros values x the hold-out cases of both sides, the
all-held case, the user mask on the generic and wide kernels, every IRLS point x every loss case x both solvers, the early stop,
and the two loss kernels on a ragged last workgroup.

Every test id names the dispatch point -- dtype, k, kernel family and how it is reached ("offset": F not 16-byte aligned; "mask":
a user mask is set) -- and cv_inputs.kernel_reached restates the conditions of cv_solve_impl (ops_cv.hip) and gives the
instantiation.  Bounds: cv_inputs.bound, relative to max|ref| -- fp32 four times the fp32 oracle's own deviation from the
restatement per class, fp64 four times the fp64 oracle's deviation from the restatement in long double (floored at 1e-12, capped
at what tests/test_gpu_cv.py allows), all measured on the CPU.  Nothing measured on a GPU sets a bound.  X carries sentinel
rows behind row ncols.

Dispatch reach (ids of test_mse_* / test_irls_* / test_cv_*):
  cv_solve_mfma32_kernel          float32-k4 / k20 / k32 -mfma32          cv_solve_mfma32x2_kernel   float32-k36 / k64 -mfma32x2
  cv_solve_mfma64_kernel          float64-k2 / k18 / k32 -mfma64
  cv_solve_kernel<float,32>       float32-k1 / k5 / k31 -reg32, float32-k32-reg32-offset, float32-k32-reg32-mask
  cv_solve_kernel<float,64>       float32-k33 / k63 -reg64, float32-k40-reg64-offset, float32-k64-reg64-mask
  cv_solve_kernel<double,32>      float64-k1 / k31 -reg32, float64-k32-reg32-offset, float64-k32-reg32-mask
  cv_solve_kernel<double,64>      float64-k33 / k64 -reg64, float64-k64-reg64-mask
  wide_cv_solve_kernel<T>         <dtype>-k65 / k100 / k128 -wide, <dtype>-k65 / k128 -wide-mask
  cv_irls_solve_kernel<T,32>      <dtype>-k6 / k32 -reg32                 cv_irls_solve_kernel<T,64>  <dtype>-k33 / k64 -reg64
  wide_cv_irls_solve_kernel<T>    <dtype>-k65 / k128 -wide
  cv_test_error_kernel<T>, cv_irls_loss_kernel<T>    test_cv_test_error / test_cv_irls_loss [<dtype>-k], k = 1, 63, 64, 65, 128
  not reached here: cv_gp_theta_rows_kernel<T> (tests/test_gpu_cv.py::test_cv_gp_theta_over_training_entries).

Largest deviation observed on an MI355X as a fraction of its bound, over the 2586 comparisons of this module (recorded, never used
as a bound): 0.30 (float32-k32-reg32, mse_robust, CD, H 0.25, zeros held out), then 0.28 and 0.28 (gamma_robust and gamma at the
same kernels); median 0.006, nine in ten below 0.15; fp64 at most 0.16 of the 1e-12 floor (k = 128, Cholesky, W side).  The sums
of the two loss kernels stay below 0.001 of their bounds: the fp32 oracle, whose deviation sets them, accumulates in fp32 and the
kernels in fp64.

Mutations, each on a scratch build with one GPU run of this module (arithmetic or a loop count only; 536 tests; the failing ones):
  last row of an odd flush dropped in mfma32 (nst = cnt >> 1)        21: every *-mfma32-* id of test_mse_case / test_mse_all_held
  (cnt + 3) >> 2 -> cnt >> 2 in mfma64                                21: every *-mfma64-* id of the same two tests
  the a11 update dropped in mfma32x2                                  14: every *-mfma32x2-* id of the same two tests
  queue remainder not moved after a flush in mfma32                   21: every *-mfma32-* id, first at H25 mz0 (33 .. 44 rows a column)
  `transposed` ignored in the hash of cv_solve_kernel                 96: every *-reg32* / *-reg64* id of test_mse_case, at W50
  second feature's correction dropped in wide_cv_solve_kernel         70: every *-wide* id of test_mse_case / test_mse_all_held
  lower-triangle mirror dropped in cv_irls_solve_kernel              124: every reg32 / reg64 id of the three IRLS tests, no wide one
  robust modifier ignored                                             54: the mse_robust and gamma_robust ids and the early stop
  1e6 cap removed from the GP weight                                  18: gp ids at every IRLS point (fp64: both solvers; fp32: Cholesky)
  fok2 terms dropped in cv_test_error_kernel                           4: test_cv_test_error at k = 65 and 128 only
  held-and-stored skip of the user-mask loop inverted                 28: every *-reg32-mask / *-reg64-mask id
"""
import numpy as np
import pytest

from tests import cv_inputs as I

pytestmark = pytest.mark.gpu

SENT = 8
SENT_X = -777.25
PREFIXES = (1, 3, 4, 5, 66)


@pytest.fixture(scope="module")
def env():
    import os
    import torch
    from rcppml_amd import _abi
    # cv_inputs.kernel_reached restates the dispatch of the shipping library; an experiment build reads this variable and would
    # send every MFMA point to the generic kernels
    assert "RCPPML_GPU_CV_VARIANT" not in os.environ
    ctx = _abi.Context(0)
    yield torch, _abi, ctx
    ctx.set_cv_mask()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _T(dtype):
    return "float" if np.dtype(dtype) == np.float32 else "double"


_DEVICE = {}


def _device_data(env, dtype, side, kind):
    key = ("D", np.dtype(dtype), side, kind)
    if key not in _DEVICE:
        D = I.data(side, kind)
        _DEVICE[key] = (D, _dev(env[0], D.p), _dev(env[0], D.i), _dev(env[0], D.x.astype(dtype)))
    return _DEVICE[key]


def _device_problem(env, dtype, k, side, offset):
    """F and G on the device, once per module, and X0 on the host.  offset: F is a view one element into a larger buffer."""
    torch = env[0]
    key = ("P", np.dtype(dtype), k, side, offset)
    if key not in _DEVICE:
        F, G, X0 = I.problem(dtype, k, side)
        if offset:
            buf = torch.zeros(F.size + 1, dtype=torch.float32 if np.dtype(dtype) == np.float32 else torch.float64, device="cuda")
            dF = buf[1:].view(F.shape)
            dF.copy_(torch.from_numpy(F))
            assert dF.data_ptr() % 16 != 0 and buf.data_ptr() % 16 == 0
        else:
            dF = _dev(torch, F)
            assert dF.data_ptr() % 16 == 0
        _DEVICE[key] = (dF, _dev(torch, G), X0)
    return _DEVICE[key]


def _device_mask(env, side, empty):
    """(mask_p, mask_i, maskT_p, maskT_i) for Context.set_cv_mask: slot 0 is the mask in A's orientation (the H side reads it),
    slot 1 its transpose (the W side)."""
    key = ("M", side, empty)
    if key not in _DEVICE:
        M = I.user_mask(side, empty)[0]
        Mt = M.transpose()
        a, b = (M, Mt) if side == "H" else (Mt, M)
        pad = lambda v: v if len(v) else np.zeros(1, np.int32)          # (an empty row list still needs a device address)
        _DEVICE[key] = tuple(_dev(env[0], v) for v in (a.p, pad(a.i), b.p, pad(b.i)))
    return _DEVICE[key]


def _finish(dX, Xpad, n):
    X = dX.cpu().numpy()
    assert np.array_equal(X[n:], Xpad[n:]), "rows behind ncols"
    X = X[:n]
    assert np.all(np.isfinite(X)), "every live row finite"
    return X


def solve_mse(env, pt, hold, mask_zeros, opt, ncols=None, cv_seed=I.CV_SEED, mode=None, empty_mask=False):
    """One MSE half-update at a dispatch point; checks the kernel reached, the sentinel rows behind ncols and finiteness."""
    torch, _abi, ctx = env
    dtype, k, pmode, fam = pt
    mode = pmode if mode is None else mode
    if mode == pmode:
        assert I.kernel_reached(dtype, k, mode != "offset", mode == "mask") == I.FAMILY_KERNEL[fam].replace("%s", _T(dtype))
    side, frac, held = I.held_for(hold)
    D, dp, di, dx = _device_data(env, dtype, side, "positive")
    dF, dG, X0 = _device_problem(env, dtype, k, side, mode == "offset")
    n = D.cols if ncols is None else ncols
    kw = I.mse_options(opt)
    Xpad = np.concatenate([X0[:n], np.full((SENT, k), SENT_X, dtype)])
    dX = _dev(torch, Xpad)
    try:
        if mode == "mask":
            ctx.set_cv_mask(*_device_mask(env, side, empty_mask))
        ctx.solve_cv(_abi.F32 if np.dtype(dtype) == np.float32 else _abi.F64, dp, di, dx, n, D.rows, dF, dG, dX, k, frac, cv_seed,
                     mask_zeros=mask_zeros, transposed=int(side == "W"), **kw)
        X = _finish(dX, Xpad, n)
    finally:
        ctx.set_cv_mask()
    if kw["nonneg"]:
        assert X.min() >= 0
    return X


def solve_irls(env, pt, case, hold, mask_zeros, solver, early=False, masked=False):
    torch, _abi, ctx = env
    dtype, k, pmode, fam = pt
    assert I.irls_kernel_reached(dtype, k) == I.IRLS_FAMILY_KERNEL[fam].replace("%s", _T(dtype))
    lt, power, robust, kind = I.LOSS_CASES[case]
    side, frac, held = I.held_for(hold)
    D, dp, di, dx = _device_data(env, dtype, side, kind)
    dF, dG, X0 = _device_problem(env, dtype, k, side, False)
    dGa = _dev(torch, I.g_add(dtype, k, solver, case))
    kw = I.irls_options(case, solver, early)
    Xpad = np.concatenate([X0, np.full((SENT, k), SENT_X, dtype)])
    dX = _dev(torch, Xpad)
    try:
        if masked:
            ctx.set_cv_mask(*_device_mask(env, side, False))
        ctx.solve_cv_irls(_abi.F32 if np.dtype(dtype) == np.float32 else _abi.F64, lt, dp, di, dx, D.cols, D.rows, dF, dGa, dX, k, frac,
                          I.CV_SEED, mask_zeros=mask_zeros, transposed=int(side == "W"), **kw)
        X = _finish(dX, Xpad, D.cols)
    finally:
        ctx.set_cv_mask()
    assert X.min() >= 0
    return X


def _check(X, Xr, bound, what):
    dev = I.deviation(X, Xr)
    print("RATIO %.4g %s" % (dev / bound, what))
    assert dev < bound, (what, dev, bound)


def _params(points, *more):
    out = []
    for pt in points:
        if not more:
            out.append(pytest.param(pt, id=I.point_id(pt)))
            continue
        for rest in more[0]:
            rest = rest if isinstance(rest, tuple) else (rest,)
            out.append(pytest.param(pt, *rest, id="-".join([I.point_id(pt)] + [str(r) for r in rest])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# MSE half-update
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt,opt", _params(I.MSE_DISPATCH, list(I.MSE_OPTIONS)))
def test_mse_case_against_reference(env, pt, opt):
    """Every dispatch point x every option case, on both mask_zeros values and the three hold-out cases (H 0.25, H 0.5, W 0.5);
    the points of mode "mask" run with the user mask of cv_inputs.user_mask set."""
    dtype, k, mode, fam = pt
    bound = I.bound(dtype, I.mse_class(k, opt))
    for hold in I.HOLD_CASES:
        for mz in (0, 1):
            Xr = I.mse_reference(dtype, k, hold, mz, opt, masked=mode == "mask")
            X = solve_mse(env, pt, hold, mz, opt)
            _check(X, Xr, bound, "%s-%s-%s-mz%d" % (I.point_id(pt), opt, hold, mz))
            if not I.mse_options(opt)["nonneg"] and Xr.min() < -10 * bound * np.abs(Xr).max():
                assert X.min() < 0                              # the clamp is really off


@pytest.mark.parametrize("pt", _params(I.MSE_DISPATCH))
def test_mse_all_held(env, pt):
    """Fraction 0.75 holds out every entry: b = 0, G_local = G - F^T F (the ridge) with zeros held out -- 131 or 67 rows through the
    queue, two flushes in one push -- and G minus the stored rows with mask_zeros; nonneg = 0, three sweeps from a non-zero X."""
    dtype, k, mode, fam = pt
    bound = I.bound(dtype, I.mse_class(k, "allheld"))
    for hold in I.ALL_HELD:
        for mz in (0, 1):
            Xr = I.mse_reference(dtype, k, hold, mz, "allheld", masked=mode == "mask")
            X = solve_mse(env, pt, hold, mz, "allheld")
            _check(X, Xr, bound, "%s-allheld-%s-mz%d" % (I.point_id(pt), hold, mz))


@pytest.mark.parametrize("pt", _params(I.MSE_DISPATCH))
def test_mse_prefix_repeat_and_seed(env, pt):
    """Two runs are bitwise equal; a run on the first n columns (n around the four-column workgroup, and 66) equals the full
    run's rows bit for bit; cv_seed = 0 gives the bits of 12345 and cv_seed = 2^32 + 77 those of 77."""
    for hold, mz in (("H50", 0), ("W50", 1)):
        X = solve_mse(env, pt, hold, mz, "cd")
        assert np.array_equal(X, solve_mse(env, pt, hold, mz, "cd"))
        for n in PREFIXES:
            assert np.array_equal(solve_mse(env, pt, hold, mz, "cd", ncols=n), X[:n]), (hold, n)
        assert np.array_equal(solve_mse(env, pt, hold, mz, "cd", cv_seed=(1 << 32) + 77), X)
        X0 = solve_mse(env, pt, hold, mz, "cd", cv_seed=0)
        assert np.array_equal(X0, solve_mse(env, pt, hold, mz, "cd", cv_seed=12345)) and not np.array_equal(X0, X)


@pytest.mark.parametrize("pt", _params([p for p in I.MSE_DISPATCH if p[2] == "mask"]))
def test_empty_user_mask_equals_the_unmasked_generic_run(env, pt):
    """A mask without entries changes no bit of the generic / wide kernel's result (the unmasked run of the same kernel: F off
    alignment where the aligned unmasked run would take an MFMA kernel)."""
    dtype, k, mode, fam = pt
    plain = "" if I.kernel_reached(dtype, k, True, False) == I.kernel_reached(dtype, k, True, True) else "offset"
    assert I.kernel_reached(dtype, k, plain != "offset", False) == I.kernel_reached(dtype, k, True, True)
    for hold in I.HOLD_CASES:
        for mz in (0, 1):
            for opt in ("cd", "chol"):
                a = solve_mse(env, pt, hold, mz, opt, empty_mask=True)
                assert np.array_equal(a, solve_mse(env, pt, hold, mz, opt, mode=plain)), (hold, mz, opt)


# ---------------------------------------------------------------------------------------------------------------------------
# IRLS half-update
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt,case,solver", _params(I.IRLS_DISPATCH, [(c, s) for c in I.LOSS_CASES for s in (0, 1)]))
def test_irls_case_against_reference(env, pt, case, solver):
    """Every IRLS point x every loss case x both solvers, on both mask_zeros values and both sides, irls_tol = 0 (every column takes
    irls_max_iter passes), with the feature term G_add."""
    dtype, k, mode, fam = pt
    bound = I.bound(dtype, I.irls_class(k, solver, case))
    for hold in I.IRLS_HOLDS:
        for mz in (0, 1):
            Xr = I.irls_reference(dtype, k, case, hold, mz, solver)[0]
            X = solve_irls(env, pt, case, hold, mz, solver)
            _check(X, Xr, bound, "%s-%s-s%d-%s-mz%d" % (I.point_id(pt), case, solver, hold, mz))


@pytest.mark.parametrize("pt", _params(I.IRLS_DISPATCH))
def test_irls_user_mask(env, pt):
    """The user mask in the IRLS kernels (Gamma, CD): masked rows leave the training entries on both sides."""
    dtype, k, mode, fam = pt
    bound = I.bound(dtype, I.irls_class(k, 0, "gamma"))
    for hold in I.IRLS_HOLDS:
        for mz in (0, 1):
            Xr = I.irls_reference(dtype, k, "gamma", hold, mz, 0, masked=True)[0]
            assert I.deviation(I.irls_reference(dtype, k, "gamma", hold, mz, 0)[0], Xr) > 100 * bound       # the mask matters
            X = solve_irls(env, pt, "gamma", hold, mz, 0, masked=True)
            _check(X, Xr, bound, "%s-gamma-masked-%s-mz%d" % (I.point_id(pt), hold, mz))


@pytest.mark.parametrize("pt", _params([p for p in I.IRLS_DISPATCH if p[1] in (32, 64, 128)]))
def test_irls_early_stop(env, pt):
    """irls_tol > 0 on the case of cv_inputs.EARLY_CASE, one point per kernel family: the columns the float64 restatement marks
    decisive (at least 95 % of them) under the class bound."""
    dtype, k, mode, fam = pt
    case, hold, mz, solver = I.EARLY_CASE
    Xr, passes, stat, trace = I.irls_reference(dtype, k, case, hold, mz, solver, early=True)
    dec = I.decisive_columns(dtype, k)
    assert dec.mean() >= 0.95
    X = solve_irls(env, pt, case, hold, mz, solver, early=True)
    _check(X[dec], Xr[dec], I.bound(dtype, I.irls_class(k, solver, case)) * np.abs(Xr).max() / np.abs(Xr[dec]).max(),
           "%s-early" % I.point_id(pt))


# ---------------------------------------------------------------------------------------------------------------------------
# Loss kernels: 67 columns, so the last workgroup of four columns is ragged
# ---------------------------------------------------------------------------------------------------------------------------
def _loss_args(env, dtype, k, kind):
    key = ("L", np.dtype(dtype), k)
    if key not in _DEVICE:
        _DEVICE[key] = tuple(_dev(env[0], a) for a in I.loss_problem(dtype, k))
    return _device_data(env, dtype, "H", kind), _DEVICE[key]


@pytest.mark.parametrize("k", I.LOSS_KS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_cv_test_error(env, dtype, k):
    torch, _abi, ctx = env
    (A, dp, di, dx), (dW, dd, dH, dth) = _loss_args(env, dtype, k, "positive")
    bound = I.bound(dtype, ("sum", "error"))
    for mz in (0, 1):
        sq_ref, n_ref = I.error_reference(dtype, k, mz)
        out = torch.zeros((2,), dtype=torch.float64, device="cuda")
        ctx.cv_test_error(_abi.F32 if dtype == np.float32 else _abi.F64, dp, di, dx, A.cols, A.rows, dW, dd, dH, k, I.LOSS_HOLD,
                          I.CV_SEED, mz, out)
        sq, cnt = out.cpu().numpy()
        assert cnt == n_ref and n_ref > 0
        print("RATIO %.4g cv_test_error-%s-k%d-mz%d" % (abs(sq - sq_ref) / abs(sq_ref) / bound, np.dtype(dtype).name, k, mz))
        assert abs(sq - sq_ref) < bound * abs(sq_ref), (mz, sq, sq_ref)


@pytest.mark.parametrize("loss_type", sorted(I.LOSS_TYPES))
@pytest.mark.parametrize("k", I.LOSS_KS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_cv_irls_loss(env, dtype, k, loss_type):
    """Counts exactly equal, n_train + n_test = the entries visited, sums within the bound; also with the user mask set."""
    torch, _abi, ctx = env
    kind, power = I.LOSS_TYPES[loss_type]
    (A, dp, di, dx), (dW, dd, dH, dth) = _loss_args(env, dtype, k, kind)
    bound = I.bound(dtype, ("sum", loss_type))
    nmask = I.user_mask("H")[1]
    S = np.zeros((A.rows, A.cols), bool)
    S[A.i, np.repeat(np.arange(A.cols), np.diff(A.p))] = True
    for masked in (False, True):
        for mz in (0, 1):
            ref = I.loss_reference(dtype, k, loss_type, mz, masked)
            out = torch.zeros((4,), dtype=torch.float64, device="cuda")
            try:
                if masked:
                    ctx.set_cv_mask(*_device_mask(env, "H", False))
                ctx.cv_irls_loss(_abi.F32 if dtype == np.float32 else _abi.F64, loss_type, dp, di, dx, A.cols, A.rows, dW, dd, dH, dth, k,
                                 I.LOSS_HOLD, I.CV_SEED, mz, power, out)
                tr, ntr, te, nte = out.cpu().numpy()
            finally:
                ctx.set_cv_mask()
            assert (ntr, nte) == (ref[1], ref[3]) and ref[3] > 0
            visited = (S if mz else np.ones_like(S)) & ~(nmask if masked else np.zeros_like(S))
            assert ntr + nte == visited.sum()
            for got, want, name in ((tr, ref[0], "train"), (te, ref[2], "test")):
                print("RATIO %.4g cv_irls_loss-%s-k%d-loss%d-mz%d-%s%s" % (abs(got - want) / abs(want) / bound, np.dtype(dtype).name, k,
                                                                        loss_type, mz, name, "-masked" if masked else ""))
                assert abs(got - want) < bound * abs(want), (masked, mz, name, got, want)
