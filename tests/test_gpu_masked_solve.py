"""rcppml_hip_solve_masked (masked_solve_kernel<T, 32>, <T, 64> and wide_masked_solve_kernel, CD and Cholesky branch each)
against the float64 restatement cd_ref.masked_half_update, at op level.  Bounds: the CD branch takes the CD bounds
(cd_inputs.cd_tolerance: fp64 1e-9; fp32 3e-4, x 4 above k = 64; x 10 without non-negativity), the Cholesky branch test_chol_clip's
5e-4 / 1e-10 -- all relative to max|ref|.  The Gram carries a ridge (cd_inputs.masked_gram): 90 rows give a singular Gram from
k = 90 on, and the mask takes rows away."""
import numpy as np
import pytest

from tests import cd_inputs as I
from tests import cd_ref as R

pytestmark = pytest.mark.gpu

SENT_X = -777.25


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_PROBLEMS = {}


def _problem(k, dtype):
    key = (k, np.dtype(dtype))
    if key not in _PROBLEMS:
        A, M, F, X0 = I.masked_problem(k, seed=50 + k)
        F, X0 = F.astype(dtype), X0.astype(dtype)
        Ad = I.Pattern(A.rows, A.cols, A.p, A.i, A.x.astype(dtype).astype(np.float64))     # the values the kernel sees
        _PROBLEMS[key] = (Ad, M, F, X0, I.masked_gram(F, dtype))
    return _PROBLEMS[key]


def _bound(dtype, k, solver_mode, nonneg):
    if solver_mode == 1:
        return 5e-4 if np.dtype(dtype) == np.float32 else 1e-10
    return I.cd_tolerance(dtype, k, nonneg)


def _run(env, dtype, A, M, F, G, Xbuf, ncols, k, **kw):
    torch, _abi, ctx = env
    dX = _dev(torch, Xbuf)
    ctx.solve_masked(_abi.F32 if np.dtype(dtype) == np.float32 else _abi.F64, _dev(torch, A.p[:ncols + 1]), _dev(torch, A.i),
                     _dev(torch, A.x.astype(dtype)), _dev(torch, M.p[:ncols + 1]), _dev(torch, M.i), ncols, _dev(torch, F),
                     _dev(torch, G), dX, k, **kw)
    return dX.cpu().numpy()


@pytest.mark.parametrize("warm", [0, 1])
@pytest.mark.parametrize("solver_mode", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [1, 8, 32, 33, 64, 65, 128])
def test_masked_half_update(env, k, dtype, solver_mode, warm):
    """37 columns (ncols % 4 != 0: the last workgroup of the 4-columns-per-block kernels is ragged) with an empty column, a column
    whose stored entries are all masked, masked rows without a stored entry and an empty mask; cold and warm, with and without
    L1 / L2, with and without non-negativity."""
    A, M, F, X0, G = _problem(k, dtype)
    edge = M.p[1] > M.p[0] and A.p[1] == A.p[0] and M.p[4] == M.p[3]
    assert edge and A.cols == 37
    for l1, l2 in ((0.0, 0.0), (0.02, 0.03)):
        for nonneg in (1, 0):
            l1q, l2q = I.q(l1, dtype), I.q(l2, dtype)
            tolq = I.q(1e-8, dtype)
            ref = R.masked_half_update(A, M, F, G, X0, l1=l1q, l2=l2q, nonneg=bool(nonneg), maxit=100, tol=tolq,
                                       solver_mode=solver_mode, warm=bool(warm))
            X = _run(env, dtype, A, M, F, G, X0, A.cols, k, l1=l1, l2=l2, nonneg=nonneg, cd_maxit=100, cd_tol=1e-8,
                     solver_mode=solver_mode, warm=warm)
            dev = np.abs(X.astype(np.float64) - ref).max() / np.abs(ref).max()
            bound = _bound(dtype, k, solver_mode, bool(nonneg))
            print("dev/bound %.3g" % (dev / bound), warm, l1, nonneg)
            assert dev < bound, (warm, l1, l2, nonneg, dev, bound)
            if nonneg:
                assert X.min() >= 0
            if l1 == 0 and nonneg and not (warm and solver_mode == 0):
                assert np.all(X[0] == 0) and np.all(X[1] == 0)       # no unmasked entry: b = 0, the solution is 0


@pytest.mark.parametrize("solver_mode", [0, 1])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [8, 64, 128])
def test_masked_single_column_and_sentinels(env, k, dtype, solver_mode):
    """ncols = 1 (column 2 of the problem: masked rows with and without a stored entry) with sentinel rows behind X."""
    A, M, F, X0, G = _problem(k, dtype)
    j = 2
    A1 = I.Pattern(A.rows, 1, [0, A.p[j + 1] - A.p[j]], A.i[A.p[j]:A.p[j + 1]], A.x[A.p[j]:A.p[j + 1]])
    M1 = I.Pattern(A.rows, 1, [0, M.p[j + 1] - M.p[j]], M.i[M.p[j]:M.p[j + 1]], M.x[M.p[j]:M.p[j + 1]])
    Xbuf = np.concatenate([X0[j:j + 1], np.full((8, k), SENT_X, dtype)])
    ref = R.masked_half_update(A1, M1, F, G, X0[j:j + 1], l1=I.q(0.02, dtype), l2=I.q(0.03, dtype), nonneg=True, maxit=100,
                               tol=I.q(1e-8, dtype), solver_mode=solver_mode, warm=True)
    X = _run(env, dtype, A1, M1, F, G, Xbuf, 1, k, l1=0.02, l2=0.03, nonneg=1, cd_maxit=100, cd_tol=1e-8, solver_mode=solver_mode, warm=1)
    assert np.array_equal(X[1:], Xbuf[1:])
    dev = np.abs(X[:1].astype(np.float64) - ref).max() / np.abs(ref).max()
    assert dev < _bound(dtype, k, solver_mode, True), dev
