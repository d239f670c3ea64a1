"""CPU-only conditions of the cross-validation matrix (tests/test_gpu_cv_matrix.py): the numpy restatement tests/cv_ref.py equals
the fp64 oracle (with and without the user mask, through the oracle's *_masked exports), the hash equals the pinned vectors and
truncates as the reference does, the edge matrix and the hold-out cases contain the edges they are meant to contain, and the
bounds of tests/cv_inputs.py are four times the oracles' own deviations.  No GPU, no torch."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import cv_inputs as I
from tests import cv_ref as R

RESTATEMENT_BOUND = 1e-12
V = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors.npz"))
f32, f64 = np.float32, np.float64


def _oc(D):
    return O.Csc((D.rows, D.cols), D.p, D.i, D.x)


def oracle_mse(dtype, k, hold, mz, opt, masked=False, cv_seed=I.CV_SEED):
    side, frac, held = I.held_for(hold)
    F, G, X0 = I.problem(dtype, k, side)
    kw = I.mse_options(opt)
    return O.cv_half_update(_oc(I.data(side)), F, G, X0, k, frac, cv_seed, mask_zeros=bool(mz), transposed=side == "W", L1=kw["l1"],
                            nonneg=bool(kw["nonneg"]), cd_maxit=kw["cd_maxit"], solver_mode=kw["solver_mode"], dtype=dtype,
                            mask=I.user_mask(side)[0] if masked else None)


def oracle_irls(dtype, k, case, hold, mz, solver, masked=False, early=False, irls_max_iter=None):
    side, frac, held = I.held_for(hold)
    lt, power, robust, kind = I.LOSS_CASES[case]
    F, G, X0 = I.problem(dtype, k, side)
    kw = I.irls_options(case, solver, early)
    return O.cv_irls_half_update(_oc(I.data(side, kind)), F, X0, k, frac, I.CV_SEED, lt, G_add=I.g_add(dtype, k, solver, case),
                                 mask_zeros=bool(mz), transposed=side == "W", L1=kw["l1"], nonneg=True, cd_maxit=kw["cd_maxit"],
                                 solver_mode=solver, irls_max_iter=irls_max_iter or kw["irls_max_iter"], irls_tol=kw["irls_tol"],
                                 power=power, robust=robust, dtype=dtype, mask=I.user_mask(side)[0] if masked else None)


def oracle_loss(dtype, k, loss_type, mz, masked=False):
    W, d, H, theta = I.loss_problem(dtype, k)
    kind, power = I.LOSS_TYPES[loss_type]
    return O.cv_explicit_loss(_oc(I.edge_matrix(kind)), W, d, H, I.LOSS_HOLD, I.CV_SEED, loss_type, theta=theta, mask_zeros=bool(mz),
                              power=power, dtype=dtype, mask=I.user_mask("H")[0] if masked else None)


def oracle_error(dtype, k, mz):
    W, d, H, theta = I.loss_problem(dtype, k)
    return O.cv_test_error(_oc(I.edge_matrix("positive")), W, d, H, I.LOSS_HOLD, I.CV_SEED, mask_zeros=bool(mz), dtype=dtype)


def _rel(a, b):
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------------------------------------------------------------------
# The hash and its truncations
# ---------------------------------------------------------------------------------------------------------------------------
def test_hash_equals_the_pinned_vectors_and_truncates_as_the_reference():
    for s in (42, 7):
        assert np.array_equal(R.cv_hash(s, V["hash_i"], V["hash_j"]), V["hash_seed%d" % s])
        seed, thr = R.mask_params(0.1, s)
        assert np.array_equal(R.cv_hash(seed, V["hash_i"], V["hash_j"]) < np.uint64(thr), V["holdout_seed%d_inv10" % s].astype(bool))
    h = lambda frac, seed=I.CV_SEED: R.holdout(I.ROWS, I.COLS, frac, seed)
    assert np.array_equal(h(0.34), h(0.5)) and not np.array_equal(h(0.34), h(1 / 3))      # (uint64)(1 / 0.34) = 2
    assert h(0.75).all() and h(0.51).all()                                               # inv_prob 1: every entry
    assert np.array_equal(h(0.25, 0), h(0.25, 12345)) and np.array_equal(h(0.25, (1 << 32) + 77), h(0.25, 77))
    assert not np.array_equal(h(0.25, 0), h(0.25, 77))
    assert np.all(h(0.5)[h(0.25)])                                                       # nested: held at 0.25 -> held at 0.5
    for i, j in ((0, 0), (130, 66), (17, 3)):
        assert int(R.cv_hash(77, i, j)) == O.cv_hash(77, i, j)


# ---------------------------------------------------------------------------------------------------------------------------
# The inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _held_counts(side, mz):
    """Per-column held-out rows (mask_zeros: held-out stored entries) over every hold-out case of the side, the all-held one included."""
    out = set()
    for hold, (s, frac) in I.HOLDS.items():
        if s == side:
            held = I.held_for(hold)[2]
            S = R.dense(I.data(side))[0]
            out |= set(((held & S) if mz else held).sum(axis=0).tolist())
    return out


def test_inputs_cover_the_edges():
    """The structural columns of cv_inputs.edge_matrix on both sides, and the held counts the MFMA queue has to get right.  With
    mask_zeros the counts are those of held-out STORED entries and the matrix sets them: 0, 1, an odd value below 32, 32, 33, every
    residue mod 4 and 64 or more on each side.  Without it the hash alone sets them (every column holds out a share of ALL rows,
    so 0 and 1 cannot occur): 31, 32 and 33, every residue mod 4, and 64 or more (H side: fraction 0.5; W side: all 67 held)."""
    lay = I.layout()
    for kind in ("positive", "counts"):
        A = I.edge_matrix(kind)
        assert (A.rows, A.cols) == (131, 67) and np.array_equal(A.x, A.x.astype(np.float32)) and np.all(A.x > 0)
        assert all(np.all(np.diff(A.i[A.p[j]:A.p[j + 1]]) > 0) for j in range(A.cols))
        At = A.transpose()
        assert all(np.all(np.diff(At.i[At.p[j]:At.p[j + 1]]) > 0) for j in range(At.cols))
    S = R.dense(I.edge_matrix())[0]
    h25, h50 = I.held_matrix(0.25), I.held_matrix(0.5)
    assert np.array_equal(S, R.dense(I.edge_matrix("counts"))[0])
    assert not S[:, I.EMPTY_COL].any() and not S[list(lay["empty_rows"])].any()
    assert S[:, lay["dense_col"]].sum() == 129 > 64 and S[lay["dense_row"]].sum() == 66 > 64
    assert (S & h25)[:, lay["dense_col"]].sum() > 32 and (S & h50)[:, lay["dense_col"]].sum() >= 64
    assert (S & h50)[lay["dense_row"]].sum() > 32
    assert S[:, I.SINGLE_COL].sum() == 1 and (S & h25)[:, I.SINGLE_COL].sum() == 1
    assert S[lay["r1"]].sum() == 1 and (S & h50)[lay["r1"]].sum() == 1
    assert S[:, I.ALLHELD_COL].sum() == 6 == (S & h25)[:, I.ALLHELD_COL].sum()
    assert S[lay["rall"]].sum() == 5 == (S & h50)[lay["rall"]].sum()
    assert [(S & h50)[:, c].sum() for c in (I.C32, I.C33, I.C31)] == [32, 33, 31]
    assert [(S & h50)[lay[r]].sum() for r in ("r32", "r33", "r31")] == [32, 33, 31]
    for side in ("H", "W"):
        assert np.all(I.problem(f32, 32, side)[2][I.CAP_COL] == 0) and np.diff(I.data(side).p)[I.CAP_COL] > 5
        c1 = _held_counts(side, 1)
        assert {0, 1, 32, 33} <= c1 and any(c % 2 == 1 and 1 < c < 32 for c in c1) and max(c1) >= 64, (side, sorted(c1))
        assert {c % 4 for c in c1 if c > 1} == {0, 1, 2, 3}
        c0 = _held_counts(side, 0)
        assert {31, 32, 33} <= c0 and {c % 4 for c in c0} == {0, 1, 2, 3} and max(c0) >= 64, (side, sorted(c0))
    c = I.held_for("H50")[2].sum(axis=0)
    assert c.min() < 64 < c.max() and ((c > 64) & (c % 32 != 0)).any()           # two flushes and a tail
    # the user masks: every kind of entry, a fully masked column, columns without an entry
    for side, hold in (("H", "H25"), ("H", "H50"), ("W", "W50")):
        M, U = I.user_mask(side)
        held = I.held_for(hold)[2]
        Sd = R.dense(I.data(side))[0]
        free = np.ones(Sd.shape[1], bool)
        free[9] = False
        for stored in (Sd, ~Sd):
            for h in (held, ~held):
                assert (U & stored & h)[:, free].any()
        assert U[:, 9].all() and not U[:, 10:16].any() and np.array_equal(R.dense(M)[0], U)
        assert I.user_mask(side, empty=True)[0].p[-1] == 0


def test_inputs_reach_the_cap_and_the_huber_modifier():
    """Weights at the 1e6 cap and below it in every capped loss case, active Huber modifiers in the robust ones (k = 32, both sides)."""
    for case, (lt, power, robust, kind) in I.LOSS_CASES.items():
        for hold in I.IRLS_HOLDS:
            for solver in (0, 1):
                trace = I.irls_reference(f32, 32, case, hold, 0, solver)[3]
                assert trace["below_cap"] and trace["capped"] == (lt != 0), (case, hold, solver)
                assert trace["huber"] == (robust > 0), (case, hold, solver)


# ---------------------------------------------------------------------------------------------------------------------------
# The restatement equals the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 33, 128])
def test_mse_restatement_equals_oracle(k):
    worst = 0.0
    for hold in I.HOLDS:
        for mz in (0, 1):
            for opt in list(I.MSE_OPTIONS) + ["allheld"]:
                for masked in (False, True):
                    d = I.deviation(oracle_mse(f64, k, hold, mz, opt, masked), I.mse_reference(f64, k, hold, mz, opt, masked))
                    worst = max(worst, d)
                    assert d < RESTATEMENT_BOUND, (hold, mz, opt, masked, d)
    assert I.deviation(oracle_mse(f64, k, "H25", 0, "cd", cv_seed=0), I.mse_reference(f64, k, "H25", 0, "cd", cv_seed=12345)) < RESTATEMENT_BOUND
    print("k = %d: worst %.2e" % (k, worst))


@pytest.mark.parametrize("k", [6, 33, 128])
def test_irls_restatement_equals_oracle(k):
    worst = 0.0
    for hold in I.IRLS_HOLDS:
        for mz in (0, 1):
            for solver in (0, 1):
                for case in I.LOSS_CASES:
                    for masked in (False, True):
                        d = I.deviation(oracle_irls(f64, k, case, hold, mz, solver, masked),
                                        I.irls_reference(f64, k, case, hold, mz, solver, masked)[0])
                        worst = max(worst, d)
                        assert d < RESTATEMENT_BOUND, (hold, mz, solver, case, masked, d)
    print("k = %d: worst %.2e" % (k, worst))


@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_loss_restatements_equal_oracle(k):
    for mz in (0, 1):
        sq, n = oracle_error(f64, k, mz)
        sr, nr = I.error_reference(f64, k, mz)
        assert n == nr and _rel(sq, sr) < RESTATEMENT_BOUND
        for lt in I.LOSS_TYPES:
            for masked in (False, True):
                o, r = oracle_loss(f64, k, lt, mz, masked), I.loss_reference(f64, k, lt, mz, masked)
                assert (o[1], o[3]) == (r[1], r[3]) and r[3] > 0
                assert _rel(o[0], r[0]) < RESTATEMENT_BOUND and _rel(o[2], r[2]) < RESTATEMENT_BOUND, (mz, lt, masked, o, r)


# ---------------------------------------------------------------------------------------------------------------------------
# The bounds
# ---------------------------------------------------------------------------------------------------------------------------
def measure(dtype, xp, mse_ks, irls_ks, loss_ks):
    """{class: (worst deviation of the `dtype` oracle from the restatement evaluated in `xp`, where)}."""
    D = {}

    def note(cls, d, where):
        if d > D.get(cls, (-1.0,))[0]:
            D[cls] = (d, where)
    for k, masked in mse_ks:
        for hold in I.HOLDS:
            for mz in (0, 1):
                for opt in (["allheld"] if hold in I.ALL_HELD else list(I.MSE_OPTIONS)):
                    d = I.deviation(oracle_mse(dtype, k, hold, mz, opt, masked), I.mse_reference(dtype, k, hold, mz, opt, masked, xp=xp))
                    note(I.mse_class(k, opt), d, (k, hold, mz, opt, masked))
    for k in irls_ks:
        for hold in I.IRLS_HOLDS:
            for mz in (0, 1):
                for solver in (0, 1):
                    for case in I.LOSS_CASES:
                        d = I.deviation(oracle_irls(dtype, k, case, hold, mz, solver), I.irls_reference(dtype, k, case, hold, mz, solver, xp=xp)[0])
                        note(I.irls_class(k, solver, case), d, (k, hold, mz))
                d = I.deviation(oracle_irls(dtype, k, "gamma", hold, mz, 0, masked=True),
                                I.irls_reference(dtype, k, "gamma", hold, mz, 0, masked=True, xp=xp)[0])
                note(I.irls_class(k, 0, "gamma"), d, (k, hold, mz, "masked"))
        if k in (32, 64, 128):
            case, hold, mz, solver = I.EARLY_CASE
            dec = I.decisive_columns(dtype, k)
            Xr = I.irls_reference(dtype, k, case, hold, mz, solver, early=True, xp=xp)[0]
            Xo = oracle_irls(dtype, k, case, hold, mz, solver, early=True)
            note(I.irls_class(k, solver, case), I.deviation(Xo[dec], Xr[dec]) * np.abs(Xr[dec]).max() / np.abs(Xr).max(), (k, "early"))
    for k in loss_ks:
        for mz in (0, 1):
            note(("sum", "error"), _rel(oracle_error(dtype, k, mz)[0], I.error_reference(dtype, k, mz, xp=xp)[0]), (k, mz))
            for lt in I.LOSS_TYPES:
                for masked in (False, True):
                    o, r = oracle_loss(dtype, k, lt, mz, masked), I.loss_reference(dtype, k, lt, mz, masked, xp=xp)
                    note(("sum", lt), max(_rel(o[0], r[0]), _rel(o[2], r[2])), (k, mz, masked))
    return D


def _report(D, table, name, subset=False):
    for cls in sorted(D, key=str):
        print("    %r: %.2e,%s# at %s" % (cls, D[cls][0], " " * max(1, 50 - len(repr(cls))), D[cls][1]))
    assert set(D) <= set(table) if subset else set(D) == set(table), (name, sorted(set(D) ^ set(table), key=str))
    for cls, (d, where) in D.items():
        assert d <= table[cls] * 1.0000001, (name, cls, d, where)


def test_fp32_bounds():
    """D per class = the worst deviation of the fp32 oracle from the float64 restatement over every fp32 k of the matrix (the
    mask points with the user mask); cv_inputs.FP32_D records it and every fp32 bound is 4 D rounded up to one digit."""
    ks = sorted({(k, mode == "mask") for dt, k, mode, fam in I.MSE_DISPATCH if dt == f32})
    D = measure(f32, f64, ks, sorted({k for dt, k, mode, fam in I.IRLS_DISPATCH if dt == f32}), I.LOSS_KS)
    _report(D, I.FP32_D, "FP32_D")
    for cls in D:
        assert I.bound(f32, cls) == I.round_up_1(4 * I.FP32_D[cls]) <= 2e-2, cls


def test_fp64_bounds():
    """The fp64 oracle against the restatement in long double.  cv_inputs.FP64_D was measured at FP64_KS / FP64_IRLS_KS (the
    smallest k of every kernel family: long double costs seconds per case at the largest) and took minutes; this test measures
    again at the k of FP64_CHECK_KS and holds the table to it.  Every fp64 bound is 4 D, at least 1e-12 and at most what
    tests/test_gpu_cv.py allows; every D recorded is below 1e-13, so every fp64 bound is the floor."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    D = measure(f64, np.longdouble, [(k, False) for k in I.FP64_CHECK_KS[0]], I.FP64_CHECK_KS[1], (1, 65))
    _report(D, I.FP64_D, "FP64_D", subset=True)
    for cls in I.FP64_D:
        assert I.FP64_D[cls] < 1e-13 and I.bound(f64, cls) == 1e-12 <= I.FP64_CAP[cls[0]], cls


def test_early_stop_case_is_decisive():
    """At most 5 % of the columns of the early-stop case are non-decisive, the columns stop at more than one pass count, and on
    the decisive columns the oracle of that dtype ends where the restatement does."""
    case, hold, mz, solver = I.EARLY_CASE
    for dtype in (f32, f64):
        for k in (32, 64, 128):
            Xr, passes, stat, trace = I.irls_reference(dtype, k, case, hold, mz, solver, early=True)
            dec = I.decisive_columns(dtype, k)
            assert dec.mean() >= 0.95, (k, int((~dec).sum()))
            assert len(np.unique(passes)) >= 2 and passes.min() < I.EARLY["irls_max_iter"], np.bincount(passes)
