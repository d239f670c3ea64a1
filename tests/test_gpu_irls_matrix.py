"""rcppml_hip_solve_irls, every kernel it dispatches to, against the float64 restatement tests/irls_ref.py (pinned to the oracle
by tests/test_irls_ref_cpu.py) on the edge matrix of tests/irls_inputs.py: every dispatch point x every loss case and x every
option case, ragged column counts, the early stop with per-column pass counts, the work counters, and the four-columns-per-wave
kernel against the one-column kernel bit for bit.

Every test id names the dispatch point -- dtype, k, kernel family, and how it is reached ("cpw1" / "cpw4": the columns-per-wave
option forced; "offset": F not 16-byte aligned) -- and the loss / option case; irls_inputs.kernel_reached restates the conditions
of irls_impl (ops_irls.hip) and gives the instantiation: NB without the robust modifier takes <5> of mfma32 / mfma32q, every
other loss case <-1>.

Bounds (irls_inputs.bound, relative to max|ref| with and without the outlier's column -- irls_inputs.deviation): fp64 1e-7 (NB, GP),
1e-6 (power family, robust); fp32 four times the fp32 oracle's own deviation from the restatement per class, measured on the CPU
(irls_inputs.FP32_D).  Nothing measured on a GPU sets a bound.  The unclamped cases leave out three of the 67 columns, by the
rule of irls_inputs.kept_columns (float64 restatement alone).  X carries sentinel rows behind row ncols and is pre-filled
with the sentinel.  The early stop runs on inputs of its own (irls_inputs.EARLY_CASES: a denser matrix on which NB, GP and
MSE + robust converge, columns stopping at three pass counts or more, at most 5 % of them non-decisive in fp32).

Largest deviation observed on an MI355X as a fraction of its bound, over the 888 comparisons of test_case_against_reference and
test_early_stop (recorded, never used as a bound): 0.85 (fp32 <float,32>, gp-free, k 31: the case that sets its class's D on
the CPU), then 0.47 and 0.41; median 0.007, nine in ten below 0.1.
"""
import numpy as np
import pytest

from tests import irls_inputs as I

pytestmark = pytest.mark.gpu

SENT = 8
SENT_X = -777.25
POINTS = list(I.DISPATCH)


def _case_params(early):
    out = []
    for pt in POINTS:
        for case, opt in I.cases_at(pt[0], pt[1]):
            if ((case, opt) in I.EARLY_CASES) == early:
                out.append(pytest.param(pt, case, opt, id="%s-%s-%s" % (I.point_id(pt), case, opt)))
    return out


@pytest.fixture(scope="module")
def env():
    import os
    import torch
    from rcppml_amd import _abi
    # irls_inputs.kernel_reached restates the dispatch of the shipping library; an experiment build reads this variable and would
    # send every MFMA point to the register kernels
    assert "RCPPML_GPU_IRLS_VARIANT" not in os.environ
    ctx = _abi.Context(0)
    ctx.set_option(_abi.OPT_CD_COUNT_NOOP, 1)
    yield torch, _abi, ctx
    ctx.set_option(_abi.OPT_CD_COUNT_NOOP, 0)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DEVICE = {}


def _device_problem(env, dtype, k, case, offset):
    """The problem's arrays on the device, once per module.  offset: F is a view one element into a larger buffer."""
    torch = env[0]
    key = (np.dtype(dtype), k, case, offset)
    if key not in _DEVICE:
        A, F, G, tr, tc = I.problem(dtype, k, case)
        if offset:
            buf = torch.zeros(F.size + 1, dtype=torch.float32 if np.dtype(dtype) == np.float32 else torch.float64, device="cuda")
            dF = buf[1:].view(F.shape)
            dF.copy_(torch.from_numpy(F))
            assert dF.data_ptr() % 16 != 0 and buf.data_ptr() % 16 == 0
        else:
            dF = _dev(torch, F)
            assert dF.data_ptr() % 16 == 0
        dG = _dev(torch, G)
        assert dG.data_ptr() % 16 == 0
        _DEVICE[key] = (A, _dev(torch, A.p), _dev(torch, A.i), _dev(torch, A.x.astype(dtype)), dF, dG,
                        None if tr is None else _dev(torch, tr), None if tc is None else _dev(torch, tc))
    return _DEVICE[key]


def solve(env, pt, case, opt, ncols=None):
    """One half-update at a dispatch point.  Returns (X (ncols, k), counters, nnz of the columns solved); checks what every run
    must keep: the sentinel rows behind ncols, every row before them written, finite results."""
    torch, _abi, ctx = env
    dtype, k, mode, kern = pt
    lt, th, power, robust, kind = I.LOSS_CASES[case]
    assert I.kernel_reached(dtype, k, mode, lt, robust).startswith(
        {"mfma32": "irls_nb_mfma32_kernel", "mfma32q": "irls_nb_mfma32q_kernel", "mfma32x2": "irls_nb_mfma32x2_kernel",
         "mfma64": "irls_nb_mfma64_kernel", "reg32": "irls_nb_solve_kernel<%s,32>", "reg64": "irls_nb_solve_kernel<%s,64>",
         "wide": "wide_irls_solve_kernel"}[kern].replace("%s", "float" if np.dtype(dtype) == np.float32 else "double"))
    A, dp, di, dx, dF, dG, dtr, dtc = _device_problem(env, dtype, k, case, mode == "offset")
    n = A.cols if ncols is None else ncols
    kw = I.options(dtype, case, opt)
    Xpad = np.full((n + SENT, k), SENT_X, dtype)
    dX = _dev(torch, Xpad)
    cpw = {"cpw1": 1, "cpw4": 4}.get(mode, 0)
    try:
        ctx.set_option(_abi.OPT_IRLS_COLUMNS_PER_WAVE, cpw)
        ctx.irls_stats(reset=True)
        ctx.solve_irls(_abi.F32 if np.dtype(dtype) == np.float32 else _abi.F64, lt, dp, di, dx, n, dF, dG, dX, k, theta_row=dtr,
                       theta_col=dtc, **kw)
        st = ctx.irls_stats(reset=True)
    finally:
        ctx.set_option(_abi.OPT_IRLS_COLUMNS_PER_WAVE, 0)
    X = dX.cpu().numpy()
    assert np.array_equal(X[n:], Xpad[n:]), "rows behind ncols"
    X = X[:n]
    assert np.all(np.isfinite(X)) and not np.any(X == SENT_X), "every row written"
    return X, st, int(A.p[n])


def _check_result(X, A, kw):
    n = X.shape[0]
    if kw["nonneg"]:
        assert X.min() >= 0
    if kw["nonneg"] or kw["l1"] == 0:           # (b = 0: without the clamp the L1 term alone moves an empty column below 0)
        empty = np.nonzero(np.diff(A.p[:n + 1]) == 0)[0]
        assert len(empty) == 0 or np.all(X[empty] == 0), "empty columns"


def _ratio(dev, bnd):
    return max(dev[0] / bnd[0], dev[1] / bnd[1])


@pytest.mark.parametrize("pt,case,opt", _case_params(early=False))
def test_case_against_reference(env, pt, case, opt):
    """Every dispatch point x every loss case and every option case (irls_tol = 0: all passes run) under the class bound, and
    the work counters: passes = ncols x irls_max_iter and nonzero-passes = irls_max_iter x nnz exactly, 0 < CD sweeps <= passes x
    cd_maxit."""
    dtype, k, mode, kern = pt
    A = I.problem(dtype, k, case)[0]
    kw = I.options(dtype, case, opt)
    Xr = I.reference(dtype, k, case, opt)[0]
    X, st, nnz = solve(env, pt, case, opt)
    _check_result(X, A, kw)
    dev = I.deviation(X, Xr, case, cols=I.kept_columns(dtype, k, case, opt))
    bound = I.bound(dtype, case, kw["nonneg"], k)
    print("dev/bound %.3g" % _ratio(dev, bound))
    assert I.within(dev, bound), (dev, bound)
    assert st["irls_column_passes"] == A.cols * kw["irls_max_iter"], st
    assert st["irls_nonzero_passes"] == kw["irls_max_iter"] * nnz, st
    assert 0 < st["irls_cd_sweeps"] <= st["irls_column_passes"] * kw["cd_maxit"], st


@pytest.mark.parametrize("case", ["nb_row", "gp"])
@pytest.mark.parametrize("pt", POINTS, ids=I.point_id)
def test_column_counts(env, pt, case):
    """The first n columns for n around the 4-column blocks and the quad kernel's 16-column blocks; the columns are independent,
    so each run is compared with the reference of the columns it solved."""
    dtype, k, mode, kern = pt
    A = I.problem(dtype, k, case)[0]
    kw = I.options(dtype, case, "base")
    Xr = I.reference(dtype, k, case, "base")[0]
    bound = I.bound(dtype, case, 1, k)
    for n in (1, 3, 4, 5, 15, 16, 17, A.cols):
        X, st, nnz = solve(env, pt, case, "base", ncols=n)
        _check_result(X, A, kw)
        full = np.concatenate([X, Xr[n:]])                              # the columns not solved contribute no deviation
        dev = I.deviation(full, Xr, case)
        assert I.within(dev, bound), (n, dev, bound)
        assert st["irls_column_passes"] == n * kw["irls_max_iter"] and st["irls_nonzero_passes"] == kw["irls_max_iter"] * nnz, (n, st)


@pytest.mark.parametrize("pt,case,opt", _case_params(early=True))
def test_early_stop(env, pt, case, opt):
    """The early-stop cases of irls_inputs.EARLY_CASES: irls_tol = 1e-4 on the edge matrix (NB, GP: next to no column stops) and the
    converging cases, whose columns stop at three pass counts or more (tests/test_irls_ref_cpu.py).  Decisive columns
    (irls_inputs.decisive_columns, at least 95 % of them) under the class bound; a non-decisive column equals the reference at
    its own pass count or at a neighbouring one, within the class bound relative to the column's OWN largest entry.  Passes
    counted = the reference's sum when every column is decisive, else within irls_max_iter - 1 per non-decisive column."""
    dtype, k, mode, kern = pt
    A = I.problem(dtype, k, case)[0]
    kw = I.options(dtype, case, opt)
    Xr, passes, stat, trace = I.reference(dtype, k, case, opt)
    X, st, nnz = solve(env, pt, case, opt)
    _check_result(X, A, kw)
    bound = I.bound(dtype, case, kw["nonneg"], k)
    dec = I.decisive_columns(dtype, k, case, opt)
    dev = I.deviation(X, Xr, case, cols=dec)
    print("dev/bound %.3g, %d non-decisive" % (_ratio(dev, bound), (~dec).sum()))
    assert I.within(dev, bound), (dev, bound)
    M = kw["irls_max_iter"]
    for j in np.nonzero(~dec)[0]:
        near = [np.abs(X[j] - trace["X"][m - 1][j]).max() / np.abs(trace["X"][m - 1][j]).max()
                for m in (passes[j] - 1, passes[j], passes[j] + 1) if 1 <= m <= M]
        assert min(near) < bound[1], (j, near, bound)
    slack = (M - 1) * int((~dec).sum())
    assert abs(st["irls_column_passes"] - int(passes.sum())) <= slack, (st, int(passes.sum()), slack)
    if slack == 0:
        assert st["irls_nonzero_passes"] == int((passes * np.diff(A.p)).sum()), st
    assert 0 < st["irls_cd_sweeps"] <= st["irls_column_passes"] * kw["cd_maxit"], st


@pytest.mark.parametrize("k", [4, 16, 32])
def test_quad_equals_single_on_the_edge_matrix(env, k):
    """irls_nb_mfma32q_kernel against irls_nb_mfma32_kernel bit for bit (both instantiations of each) on the columns of 0, 1, 2,
    3, .. 63, 64, 65 and 97 stored entries, every loss and option case; the counters agree as well."""
    single, quad = (np.float32, k, "cpw1", "mfma32"), (np.float32, k, "cpw4", "mfma32q")
    for case, opt in I.cases_at(np.float32, k):
        X1, st1, _ = solve(env, single, case, opt)
        X4, st4, _ = solve(env, quad, case, opt)
        assert np.array_equal(X1, X4), (case, opt, float(np.abs(X1 - X4).max()))
        assert st1 == st4, (case, opt, st1, st4)
