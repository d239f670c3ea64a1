"""tests/cd_ref.py (the float64 restatement the GPU CD and masked-solve tests compare with) against the oracle in fp64, on the
inputs the GPU tests use: iterates <= 1e-12 relative, equal sweep counts.  Also the conditions on those inputs that the GPU
tests rely on: the fp32 oracle stays within a quarter of the fp32 bound of the restatement, and at most 5 % of the columns of
the early-exit cases are non-decisive."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import cd_inputs as I
from tests import cd_ref as R


def _oracle_cd(G, B, X0, kw, dtype):
    """The prologue of rcppml_hip_solve_cd, then O.cd_col per column, in `dtype`.  Returns (X, sweeps)."""
    n, k = B.shape
    X = np.empty((n, k), dtype)
    sw = np.empty(n, np.int64)
    for j in range(n):
        b = B[j].astype(dtype)
        if kw.get("l1_pre", 0) > 0:
            b = b - dtype(kw["l1_pre"])
        x = np.zeros(k, dtype) if kw.get("zero_init") else X0[j].astype(dtype)
        if kw.get("warm"):
            for c in range(k):
                b = b - G[c] * x[c]
        x, _, it = O.cd_col(G, b, x, L1=kw.get("l1_cd", 0.0), L2=kw.get("l2_cd", 0.0), nonneg=bool(kw.get("nonneg", 1)),
                            maxit=kw["maxit"], ub=kw.get("ub_cd", 0.0), tol=kw["tol"])
        if kw.get("ub_post", 0) > 0:
            x = np.minimum(x, dtype(kw["ub_post"]))
        X[j], sw[j] = x, it
    return X, sw


@pytest.mark.parametrize("k", I.OPTION_KS)
def test_options_match_oracle_cd_col(k):
    G, B, X0, ub, cases, refs = I.options_reference(np.float64, k)
    assert set(cases) == set(I.OPTION_NAMES)
    for name, kw in cases.items():
        Xr, sw, stat = refs[name]
        Xo, swo = _oracle_cd(G, B, X0, kw, np.float64)
        assert np.abs(Xo - Xr).max() <= 1e-12 * np.abs(Xr).max(), name
        assert np.array_equal(sw, swo) and np.all(sw == 7), name
    # the bound binds on part of the entries and leaves the rest free; L1 inside the step leaves part of the solution alive
    Xub = refs["ub_cd"][0]
    assert (Xub == ub).any() and ((Xub > 0) & (Xub < ub)).any()
    assert (refs["l1_l2_ub"][0] == ub).any()
    assert (refs["l1_cd"][0] > 0).any() and np.abs(refs["l1_cd"][0] - refs["cold"][0]).max() > 1e-3 * np.abs(refs["cold"][0]).max()
    assert (refs["free"][0] < 0).any() or k == 1
    # a 7-sweep solve is NOT always short of its fixed point: from k = 9 on between half and all of the columns still move in the
    # seventh sweep (the rest have converged exactly -- few active coordinates).  Kernels that stop at a fixed point would report
    # fewer than 7 sweeps there; the explicit variants the matrix runs all report maxit (include/rcppml_gpu.h, sweeps_out).
    if k >= 9:
        assert np.mean(refs["cold"][2][:, -1] > 0) > 0.4


@pytest.mark.parametrize("k", (9, 40, 129))
def test_batch_is_the_per_column_restatement(k):
    """cd_solve_batch only vectorises the loop over columns: bit for bit the per-column function."""
    G, B, X0, ub, cases, refs = I.options_reference(np.float64, k)
    for name in ("warm", "l1_l2_ub", "free_l2", "ub_post"):
        Xr, sw, stat = refs[name]
        for j in (0, 7, I.OPTION_N - 1):
            x, it, st = R.cd_solve(G, B[j], X0[j], **I.ref_kwargs(cases[name]))
            assert np.array_equal(x, Xr[j]) and it == sw[j] and np.array_equal(st, stat[j, :len(st)]), (name, j)
    G, B, X0, kw, (Xr, sw, stat) = I.early_reference(np.float64, 9 if k == 9 else 32, 1e-3, True)
    for j in (1, 50):
        x, it, st = R.cd_solve(G, B[j], X0[j], **I.ref_kwargs(kw))
        assert np.array_equal(x, Xr[j]) and it == sw[j] and np.array_equal(st, stat[j, :it]) and np.isnan(stat[j, it:]).all()


def test_batch_with_one_gram_per_column():
    """The form masked_half_update uses: a Gram per column, one of them with a non-positive diagonal entry (that coordinate is
    skipped in that column only).  Bit for bit the per-column function, with and without non-negativity."""
    k, n = 33, 5
    rng = np.random.default_rng(7)
    Gs = np.stack([I.cd_problem(k, 1, np.float64, 900 + j, ridge=I.EARLY_RIDGE)[0] for j in range(n)])
    Gs[2, 4, 4] = 0.0
    Gs[3, 0, 0] = -1.0
    B, X0 = rng.standard_normal((n, k)), rng.uniform(size=(n, k))
    for nonneg in (True, False):
        for warm in (True, False):
            Xb, sw, stat = R.cd_solve_batch(Gs, B, X0, warm=warm, zero_init=not warm, nonneg=nonneg, maxit=100, tol=1e-4)
            assert not nonneg or sw.min() < sw.max()           # the free solves run all 100 sweeps
            for j in range(n):
                x, it, st = R.cd_solve(Gs[j], B[j], X0[j], warm=warm, zero_init=not warm, nonneg=nonneg, maxit=100, tol=1e-4)
                assert np.array_equal(x, Xb[j]) and it == sw[j] and np.array_equal(st, stat[j, :it]), (nonneg, warm, j)
            assert Xb[2, 4] == (X0[2, 4] if warm else 0) and Xb[3, 0] == (X0[3, 0] if warm else 0)


@pytest.mark.parametrize("k", I.EARLY_KS)
def test_early_exit_matches_oracle_nnls_batch(k):
    for tol in (1e-8, 1e-3):
        for warm in (False, True):
            G, B, X0, kw, (Xr, sw, stat) = I.early_reference(np.float64, k, tol, warm)
            Xo = O.nnls_batch(G, B, X=X0 if warm else None, maxit=100, tol=tol, warm=warm)
            assert np.abs(Xo - Xr).max() <= 1e-12 * np.abs(Xr).max(), (tol, warm)
            _, swo = _oracle_cd(G, B, X0, kw, np.float64)
            assert np.array_equal(sw, swo), (tol, warm)
            assert sw.min() >= 2 and sw.min() < sw.max()        # columns leave at different sweeps


def test_input_conditions_fp32():
    """Conditions on the inputs of the GPU tests, from the CPU alone: D = deviation of the fp32 oracle from the float64
    restatement <= a quarter of the fp32 bound in every (k, option) class and at every column count, <= 5 % non-decisive columns in the early-exit cases
    (both dtypes), and the fp32 oracle's sweep counts equal to the restatement's on every decisive column.
    The figures are recorded in the docstring of tests/test_gpu_cd_matrix.py."""
    worst = {}
    for k in I.OPTION_KS:
        G, B, X0, ub, cases, refs = I.options_reference(np.float32, k)
        for name, kw in cases.items():
            Xo, _ = _oracle_cd(G, B, X0, kw, np.float32)
            Xr = refs[name][0]
            D = np.abs(Xo - Xr).max() / np.abs(Xr).max()
            frac = D / I.cd_tolerance(np.float32, k, bool(kw.get("nonneg", 1)))
            worst[k] = max(worst.get(k, 0.0), frac)
            assert frac <= 0.25, (k, name, D)
    print("options: D / bound per k:", {k: round(v, 3) for k, v in worst.items()})
    for k in I.COUNT_KS:                     # test_column_counts: every run against the columns it solved
        G, B, X0, Xr = I.count_reference(np.float32, k)
        Xo, _ = _oracle_cd(G, B, X0, dict(warm=1, maxit=7, tol=0.0), np.float32)
        for n in I.COUNT_NS:
            D = np.abs(Xo[:n] - Xr[:n]).max() / np.abs(Xr[:n]).max()
            print("column counts: k %d n %d D / bound %.3f" % (k, n, D / I.cd_tolerance(np.float32, k)))
            assert D <= 0.25 * I.cd_tolerance(np.float32, k), (k, n, D)
    shares = {}
    for dtype in (np.float32, np.float64):
        for k in I.EARLY_KS:
            for tol in (1e-8, 1e-3):
                for warm in (False, True):
                    G, B, X0, kw, (Xr, sw, stat) = I.early_reference(dtype, k, tol, warm)
                    share = 1.0 - R.decisive(stat, I.q(tol, dtype), I.EARLY_DELTA[np.dtype(dtype)]).mean()
                    shares[(np.dtype(dtype).name, k, tol, warm)] = round(float(share), 3)
                    assert share <= 0.05, (dtype, k, tol, warm, share)
                    if dtype == np.float32:
                        Xo, swo = _oracle_cd(G, B, X0, kw, np.float32)
                        D = np.abs(Xo - Xr).max() / np.abs(Xr).max()
                        assert D <= 0.25 * I.cd_tolerance(np.float32, k), (k, tol, warm, D)
                        # the reference's own error: on a decisive column the fp32 oracle must reach the float64 count, or no fp32
                        # kernel can be asked to (cd_inputs.EARLY_SEED)
                        dec = R.decisive(stat, I.q(tol, dtype), I.EARLY_DELTA[np.dtype(dtype)])
                        assert np.array_equal(swo[dec], sw[dec]), (k, tol, warm, np.nonzero(dec & (swo != sw))[0])
    print("early exit: non-decisive shares:", shares)


def _csc(P):
    return O.Csc((P.rows, P.cols), P.p, P.i, P.x)


@pytest.mark.parametrize("solver_mode", [0, 1])
@pytest.mark.parametrize("k", [1, 8, 33, 65])
def test_masked_half_update_matches_one_oracle_iteration(k, solver_mode):
    """Two iterations of O.nmf_fit with an explicit mask, no scaling (norm_type 2), unsorted: the first runs both half-updates
    cold, the second warm -- each is one masked_half_update on the previous factors.  k <= rows - masked rows keeps the Gram of
    the oracle's fit (no ridge there) positive definite on the H side."""
    A, M, F, X0 = I.masked_problem(k, seed=50 + k)
    At, Mt = A.transpose(), M.transpose()
    opts = dict(L1=(0.01, 0.02), L2=(0.03, 0.04), cd_maxit=40, cd_tol=1e-6, solver_mode=solver_mode, norm_type=2, sort_model=False,
                tol=0.0, mask=_csc(M))
    W0, H0 = F, X0
    fit1 = O.nmf_fit(_csc(A), W0, H0, np.float64, max_iter=1, **opts)
    fit2 = O.nmf_fit(_csc(A), W0, H0, np.float64, max_iter=2, **opts)
    assert fit1.iter == 1 and fit2.iter == 2
    hk = dict(l1=0.02, l2=0.04, maxit=40, tol=1e-6, solver_mode=solver_mode)
    wk = dict(l1=0.01, l2=0.03, maxit=40, tol=1e-6, solver_mode=solver_mode)

    def close(a, b):
        return np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)

    H1 = R.masked_half_update(A, M, W0, O.gram(W0), H0, warm=False, **hk)
    assert close(H1, fit1.H)
    W1 = R.masked_half_update(At, Mt, fit1.H, O.gram(fit1.H), W0, warm=False, **wk)
    assert close(W1, fit1.W_T)
    if solver_mode == 0 or k <= 33:      # the second iteration's Cholesky at k = 65 meets a Gram of rank <= 37: nothing to compare
        H2 = R.masked_half_update(A, M, fit1.W_T, O.gram(fit1.W_T), fit1.H, warm=True, **hk)
        assert close(H2, fit2.H)
        W2 = R.masked_half_update(At, Mt, fit2.H, O.gram(fit2.H), fit1.W_T, warm=True, **wk)
        assert close(W2, fit2.W_T)
