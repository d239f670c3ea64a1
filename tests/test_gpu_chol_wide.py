"""The blocked MFMA Cholesky + clip (kernels_chol_wide.hip.h: 64 < k <= 256 in fp64, 128 < k <= 256 in fp32) behind
rcppml_hip_solve_chol, against np.linalg.solve in float64.

Bound: max|X - X_ref| / max|X_ref| <= eps(dtype) * cond_2(G), the first-order forward-error scale of a backward-stable solve;
the condition number is computed here from the float64 copy of G.  A numpy emulation of the blocked scheme (working precision,
block inverses, blocks 32 / 16) sits at 0.04 - 0.07 of it on these inputs (cond 7e2 - 3e3)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CASES = [(F64, k) for k in (65, 96, 128, 129, 255, 256)] + [(F32, k) for k in (129, 255, 256)]


@functools.lru_cache(maxsize=None)
def problem(dtype, k, n):
    """G = F'F + I / 2 (F uniform, (4k + 5) x k), B = 3 N(0, 1) + 1 as (n, k), both in dtype; cond_2 of the float64 copy of G."""
    rng = np.random.default_rng(1000 * k + n)
    F = rng.uniform(size=(4 * k + 5, k))
    G = (F.T @ F + 0.5 * np.eye(k)).astype(dtype)
    B = (3 * rng.standard_normal((n, k)) + 1).astype(dtype)
    return G, B, np.linalg.cond(G.astype(F64), 2)


def reference(G, B, l1, nonneg, ub):
    X = np.linalg.solve(G.astype(F64), (B.astype(F64) - l1).T).T
    X = np.maximum(X, 0) if nonneg else X
    return np.minimum(X, ub) if ub > 0 else X


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0)


def solve(env, dtype, G, B, k, n, l1=0.1, nonneg=1, ub=0.0, pad=0):
    """X as (n + pad, k); the pad rows of B and X hold the sentinel 7 and are returned with the rest."""
    torch, _abi, ctx = env
    dB = torch.full((n + pad, k), 7.0, dtype=torch.from_numpy(B).dtype, device="cuda")
    dB[:n] = torch.from_numpy(B).cuda()
    dX = torch.full_like(dB, 7.0)
    ctx.solve_chol(_abi.F32 if dtype == F32 else _abi.F64, torch.from_numpy(G).cuda(), dB, dX, k, n, l1_pre=l1, nonneg=nonneg,
                   ub_post=ub)
    return dX.cpu().numpy(), dB.cpu().numpy()


def check(X, X_ref, dtype, cond, what):
    err, bound = np.abs(X - X_ref).max() / np.abs(X_ref).max(), np.finfo(dtype).eps * cond
    print("%s: err %.3e bound %.3e (%.3f of it), cond %.3e" % (what, err, bound, err / bound, cond))
    assert err <= bound


@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("dtype,k", CASES)
def test_solve_against_float64(env, dtype, k, n):
    G, B, cond = problem(dtype, k, n)
    X, _ = solve(env, dtype, G, B, k, n)
    assert X.min() >= 0
    check(X, reference(G, B, 0.1, 1, 0.0), dtype, cond, "k=%d n=%d %s" % (k, n, dtype.__name__))


@pytest.mark.parametrize("nonneg,ub", [(1, 0.05), (0, 0.0)])
@pytest.mark.parametrize("dtype,k", [(F64, 96), (F32, 255)])
def test_clips(env, dtype, k, nonneg, ub):
    G, B, cond = problem(dtype, k, 97)
    X, _ = solve(env, dtype, G, B, k, 97, nonneg=nonneg, ub=ub)
    X_ref = reference(G, B, 0.1, nonneg, ub)
    assert (X.min() >= 0 and X.max() <= ub) if nonneg else X.min() < 0
    check(X, X_ref, dtype, cond, "nonneg=%d ub=%g" % (nonneg, ub))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_tails_do_not_leak_and_calls_repeat(env, dtype):
    """k = 129 (a rank tail of one), 97 columns (a column tail), three sentinel rows behind B and X."""
    G, B, cond = problem(dtype, 129, 97)
    X, Bd = solve(env, dtype, G, B, 129, 97, pad=3)
    assert np.all(X[97:] == 7) and np.all(Bd[97:] == 7) and np.array_equal(Bd[:97], B)
    check(X[:97], reference(G, B, 0.1, 1, 0.0), dtype, cond, "padded")
    X2, _ = solve(env, dtype, G, B, 129, 97, pad=3)
    assert np.array_equal(X, X2)
    assert np.array_equal(X[:97], solve(env, dtype, G, B, 129, 97)[0])


@pytest.mark.parametrize("precision,k", [("fp32", 130), ("fp64", 70)])
def test_nmf_default_solver(precision, k):
    """nmf() with the default solver reaches the blocked path (auto = Cholesky above rank 32).  Checked against the float64
    numpy restatement of the same three Cholesky + clip iterations from the same start, at the solve's bound with the largest
    cond_2 among the six Grams the restatement meets.  NOT against the CD fit's loss: solve-then-clip is not NNLS, and on this
    input its loss after three iterations is 9.4 x (k = 130) and 2.7 x (k = 70) that of CD run to convergence (CPU oracle,
    float64), far outside the solver-to-solver margins; the CD call stays as the second fit from the same start."""
    import scipy.sparse as sp
    from rcppml_amd import nmf as N
    from rcppml_amd.data import r_runif
    A = sp.random(300, 280, density=0.1, format="csc", random_state=np.random.default_rng(5), dtype=np.float64)
    mod = N.nmf(A, k, maxit=3, tol=0, seed=7, precision=precision)
    cd = N.nmf(A, k, maxit=3, tol=0, seed=7, precision=precision, solver="cd", cd_maxit=1000, cd_tol=1e-12)
    assert mod.misc["solver"] == "cholesky" and cd.misc["solver"] == "cd"
    assert np.isfinite(mod.misc["loss"]) and np.isfinite(cd.misc["loss"])
    assert mod.w.min() >= 0 and mod.h.min() >= 0 and mod.d.min() >= 0
    Ad, W, conds = A.toarray(), r_runif(7, 300 * k).reshape(k, 300).T, []
    for half in range(6):                                  # H from W, W from H, each followed by the L1 scaling into d
        F, M = (W, Ad.T) if half % 2 == 0 else (H, Ad)
        G = F.T @ F + 1e-15 * np.eye(k)
        conds.append(np.linalg.cond(G, 2))
        X = np.maximum(np.linalg.solve(G, (M @ F).T).T, 0)
        d = np.abs(X).sum(0) + 1e-15
        H, W = (X / d, W) if half % 2 == 0 else (H, X / d)
    o = np.argsort(-d, kind="stable")
    dtype = F32 if precision == "fp32" else F64
    for name, got, ref in (("w", mod.w, W[:, o]), ("d", mod.d, d[o]), ("h", mod.h, H[:, o].T)):
        check(got, ref, dtype, max(conds), "%s k=%d %s" % (precision, k, name))
