"""CPU-only conditions of the IRLS half-update matrix (tests/test_gpu_irls_matrix.py): the float64 restatement tests/irls_ref.py
equals the oracle, the fp32 bounds of tests/irls_inputs.py are four times the fp32 oracle's own deviation, the early-stop inputs
are decisive, and the inputs contain the edges they are meant to contain.  No GPU, no torch.

Measured here (CPU, recorded, asserted below):
  restatement against the fp64 oracle, every loss and option case at k = 5, 32, 100, iterate after every pass count of the
  early-stop cases included: worst deviation 1.3e-12 of max|ref| without the outlier's column, 1.9e-9 with it (the weighted Gram and the reconstruction are summed by
  numpy.einsum, not in the oracle's loop order); bound 1e-10, and 1e-8 on the outlier's column, whose eight passes of the NB
  early-stop case swing between two states and amplify the difference.
  D per class and the fp32 bounds: irls_inputs.FP32_D.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import cd_ref
from tests import irls_inputs as I
from tests.cd_inputs import q

RESTATEMENT_BOUND = (1e-8, 1e-10)           # with the outlier's column, without it (irls_inputs.deviation)
F32_KS = sorted({k for dt, k, mode, kern in I.DISPATCH if np.dtype(dt) == np.float32})


def oracle_run(dtype, k, case, opt, irls_max_iter=None):
    A, F, G, tr, tc = I.problem(dtype, k, case)
    kw = I.options(dtype, case, opt)
    Ao = O.Csc((A.rows, A.cols), A.p, A.i, A.x)
    return O.irls(I.LOSS_CASES[case][0], Ao, F, G, k, L1=kw["l1"], L2=kw["l2"], nonneg=bool(kw["nonneg"]), cd_maxit=kw["cd_maxit"],
                  irls_max_iter=irls_max_iter or kw["irls_max_iter"], irls_tol=kw["irls_tol"], theta_row=tr, theta_col=tc,
                  dtype=dtype, power=kw["loss_param"], robust=kw["robust_delta"])


def passes_from_iterates(Xs):
    """Pass counts read off the iterates after 1, 2, .. M passes at most (the oracle returns no counts): the first m from which
    on a column no longer changes.  (A column whose pass m + 1 moves nothing at all stops there, after m + 1 passes, with the
    iterate of pass m: the count read off is m.  The same rule is applied to both sides.)"""
    M = len(Xs)
    differs = np.stack([np.any(Xs[m] != Xs[M - 1], axis=1) for m in range(M)])
    return M - np.argmax(differs[::-1], axis=0) + 1 - np.where(differs.any(axis=0), 0, M)


@pytest.mark.parametrize("k", [5, 32, 100])
def test_restatement_equals_oracle(k):
    """fp64 on both sides; the NB cases through O.irls_nb as well.  The early-stop cases are compared after every pass count
    1 .. irls_max_iter (the oracle run with that limit against the restatement's iterate history): a column stopped one pass
    early or late on either side would show as a deviation of the size of a pass's step."""
    worst = np.zeros(2)
    for case, opt in I.all_cases():
        Xr, passes, stat, trace = I.reference(np.float64, k, case, opt)
        d = I.deviation(oracle_run(np.float64, k, case, opt), Xr, case)
        if (case, opt) in I.EARLY_CASES:
            M = I.options(np.float64, case, opt)["irls_max_iter"]
            Xo = [oracle_run(np.float64, k, case, opt, irls_max_iter=m) for m in range(1, M + 1)]
            d = tuple(np.max([d] + [I.deviation(Xo[m], trace["X"][m], case) for m in range(M)], axis=0))
            assert np.array_equal(passes_from_iterates(Xo), passes_from_iterates(trace["X"])), (case, opt)
            assert np.array_equal(passes_from_iterates(trace["X"]), passes), (case, opt)
        if I.LOSS_CASES[case][0] == 5 and I.LOSS_CASES[case][3] == 0:
            A, F, G, tr, tc = I.problem(np.float64, k, case)
            kw = I.options(np.float64, case, opt)
            Xn = O.irls_nb(O.Csc((A.rows, A.cols), A.p, A.i, A.x), F, G, k, L1=kw["l1"], L2=kw["l2"], nonneg=bool(kw["nonneg"]),
                           cd_maxit=kw["cd_maxit"], irls_max_iter=kw["irls_max_iter"], irls_tol=kw["irls_tol"], theta_row=tr, theta_col=tc)
            d = tuple(np.maximum(d, I.deviation(Xn, Xr, case)))
        print("k = %d %s/%s: %.2e %.2e" % (k, case, opt, *d))
        worst = np.maximum(worst, d)
        assert I.within(d, RESTATEMENT_BOUND), (case, opt, d)
    print("worst", worst)


@pytest.fixture(scope="module")
def fp32_deviation():
    """{(k, case, opt): deviation of the fp32 oracle from the restatement on the fp32-rounded inputs}, every fp32 k of the matrix."""
    out = {}
    for k in F32_KS:
        for case, opt in I.cases_at(np.float32, k):
            Xr = I.reference(np.float32, k, case, opt)[0]
            cols = I.kept_columns(np.float32, k, case, opt)
            if (case, opt) in I.EARLY_CASES:
                cols = cols & I.decisive_columns(np.float32, k, case, opt)
            out[(k, case, opt)] = I.deviation(oracle_run(np.float32, k, case, opt), Xr, case, cols=cols)
    return out


def test_fp32_bounds(fp32_deviation):
    """D per class = worst deviation of the fp32 oracle from the restatement, with and without the outlier's column
    (irls_inputs.deviation); each class bound is 4 D rounded up to one digit (irls_inputs.FP32_D / FP32_BOUND) and stays under
    the 3e-2 the suite allowed so far.  The unclamped cases are classes of their own; irls_inputs.kept_columns leaves three of
    their 67 columns out, by a rule on the float64 restatement alone."""
    D = {}
    for (k, case, opt), d in fp32_deviation.items():
        cls = I.bound_class(case, I.options(np.float32, case, opt)["nonneg"], k)
        for s in (0, 1):
            if d[s] > D.get((cls, s), (0.0,))[0]:
                D[(cls, s)] = (d[s], k, case, opt)
    for cls, s in sorted(D):
        print("%-30s %s D = %.2e at k = %d %s/%s   recorded %.2e bound %.0e" % (
            cls, ("all ", "rest")[s], *D[(cls, s)], I.FP32_D.get(cls, (np.nan,) * 2)[s], I.FP32_BOUND.get(cls, (np.nan,) * 2)[s]))
    assert {c for c, s in D} == set(I.FP32_D)
    for (cls, s), (d, k, case, opt) in D.items():
        assert I.FP32_BOUND[cls][s] == I.round_up_1(4 * I.FP32_D[cls][s])
        assert d <= I.FP32_BOUND[cls][s] / 4, (cls, s, d, k, case, opt)
        assert I.FP32_BOUND[cls][s] <= 3e-2, cls
    for case, opt in I.all_cases():
        assert I.kept_columns(np.float32, 32, case, opt).mean() >= 0.95


ORACLE_KS = {np.dtype(np.float32): (4, 16, 31, 48, 65, 128), np.dtype(np.float64): (2, 16, 33, 65)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_early_stop_inputs_are_decisive(dtype):
    """irls_inputs.decisive_columns: at most 5 % of the columns of any early-stop case are non-decisive, at every k of the matrix;
    in the converging cases (irls_inputs.CONVERGING) the non-empty columns stop at three different pass counts or more, so that a
    kernel's `rel < irls_tol` break is taken at several passes.  On the decisive columns the oracle of that dtype stops after the
    restatement's number of passes (else no kernel of that dtype can be held to it); checked at the k of ORACLE_KS, the smallest
    and the largest of the kernels.  Seed changes: irls_inputs.DENSE_F_SHIFT."""
    for k in sorted({k for dt, k, mode, kern in I.DISPATCH if np.dtype(dt) == np.dtype(dtype)}):
        for case, opt in I.EARLY_CASES:
            Xr, passes, stat, trace = I.reference(dtype, k, case, opt)
            M = I.options(dtype, case, opt)["irls_max_iter"]
            dec = I.decisive_columns(dtype, k, case, opt)
            assert dec.mean() >= 0.95, (k, case, opt, int((~dec).sum()))
            if (case, opt) in I.CONVERGING:
                nonempty = np.diff(I.problem(dtype, k, case)[0].p) > 0
                assert len(np.unique(passes[nonempty])) >= 3, (k, case, np.bincount(passes[nonempty]))
            if k not in ORACLE_KS[np.dtype(dtype)]:
                continue
            Xo = [oracle_run(dtype, k, case, opt, irls_max_iter=m) for m in range(1, M + 1)]
            po = passes_from_iterates(Xo)
            pr = passes_from_iterates(trace["X"])
            assert np.array_equal(po[dec], pr[dec]), (k, case, np.nonzero(dec & (po != pr))[0])
            if np.dtype(dtype) == np.float32 and (case, opt) in I.CONVERGING:
                err = np.abs(Xo[-1] - Xr).max(axis=1) / np.maximum(np.abs(Xr).max(axis=1), 1e-300)
                print("k = %d %s/%s: fp32 oracle, worst column %.2e of its largest entry" % (k, case, opt, err[dec].max()))


def test_inputs_cover_the_edges():
    """The edge matrix holds every listed column length, sorted rows and the outlier; every feature is strictly positive in some
    column of the reference; weights at the 1e6 cap and below it; active Huber modifiers in the robust cases."""
    for kind in ("counts", "positive"):
        A = I.edge_matrix(kind)
        cnt = np.diff(A.p)
        assert tuple(cnt[:len(I.EDGE_COUNTS)]) == I.EDGE_COUNTS and cnt[len(I.EDGE_COUNTS):].min() >= 5 and cnt.max() == I.ROWS
        assert all(np.all(np.diff(A.i[A.p[j]:A.p[j + 1]]) > 0) for j in range(A.cols))
        assert np.all(A.x > 0) and A.x.max() > 300 * np.median(A.x) and np.array_equal(A.x, A.x.astype(np.float32))
        if kind == "counts":
            assert np.array_equal(A.x, np.round(A.x))
        At = A.transpose()
        assert all(np.all(np.diff(At.i[At.p[j]:At.p[j + 1]]) > 0) for j in range(At.cols)) and At.p[-1] == A.p[-1]
    for dt, k, mode, kern in I.DISPATCH:
        X = I.reference(dt, k, "nb_row", "base")[0]
        assert np.all((X > 0).any(axis=0)), (np.dtype(dt).name, k)
    k = 32
    for case, (lt, th, power, robust, kind) in I.LOSS_CASES.items():
        trace = I.reference(np.float32, k, case, "base")[3]
        w = [x[np.isfinite(x)] for x in trace["w"]]
        if lt >= 5 and not robust > 0:
            # x starts at 0: every reconstruction of the first pass is 0 and every weight of it sits at the cap; below the cap from
            # the second pass on
            assert np.all(w[0] == 1e6) and (len(w) == 1 or (w[1] < 1e6).any()), case
        if case in ("gamma", "invgauss"):
            assert (np.concatenate(w[1:]) == 1e6).any(), case                    # the cap binds beyond the first pass as well
        if robust > 0:
            assert all(h.any() for h in trace["huber"]) and not all(h[trace["ok"]].all() for h in trace["huber"]), case
