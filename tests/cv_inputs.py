"""Shared inputs of tests/test_cv_ref_cpu.py and tests/test_gpu_cv_matrix.py: the edge matrix, the hold-out cases, the user masks,
the factor matrices, the option and loss cases, the dispatch points of rcppml_hip_solve_cv / rcppml_hip_solve_cv_irls, the bounds
and the references of tests/cv_ref.py, computed once per process and shared.  numpy only: no torch, no GPU code, no oracle."""
import numpy as np

from tests import cv_ref as R
from tests.cd_inputs import Pattern, q
from tests.irls_inputs import round_up_1

ROWS, COLS = 131, 67                # 131 = 2 x 64 + 3 rows; 67 = 64 + 3 columns: the last workgroup of four has three live waves
CV_SEED = 77
MATRIX_SEED = 5
# designated columns of the edge matrix (H side) ...
EMPTY_COL, SINGLE_COL, ALLHELD_COL, CAP_COL, C32, C33, C31 = 0, 2, 3, 4, 5, 6, 7
FIRST_FREE = 8                      # ... columns from here on are random, one of them (layout()["dense_col"]) dense
RIDGE = 0.25                        # on the MSE Gram, a fraction of its mean diagonal (cd_inputs.masked_gram): see BOUNDS
# The IRLS feature term G_add = ridge I + 0.01 1 1^T.  CD (six sweeps) is not sensitive to the conditioning of G_w and takes ridge 0.5.
# Cholesky is: a weight at the 1e6 cap next to G_add = O(1) gives G_w a condition number of 1e6 |f|^2 / ridge and more -- on the W
# side at k = 128 there are fewer training rows than features -- and the fp32 ORACLE itself then ends in 1e29 or NaN.  With ridge
# 1e5 the capped passes keep a condition number of ~ 1e2 and the fp32 oracle stays within 7e-5 of the restatement at every k,
# while 1e6 f f^T still outweighs the ridge, so the weighted Gram decides the result.  MSE + robust has weights <= 1: ridge 0.5.
G_ADD_RIDGE = {"cd": 0.5, "chol": 1e5}

# Hold-out cases: name -> (side, fraction).  Held-out rows per column with zeros held out (the hash alone decides), cv_seed = 77:
#   H 0.25: 19..44 (31, 32, 33 among them)   H 0.5: 52..81 (counts that cross 64: two queue flushes and a tail)
#   W 0.5:  22..44 (31, 32, 33 among them, every residue mod 4)
# "all" holds out every entry (0.75 -> inv_prob 1): with zeros held out the flush loop runs twice in one push of 64 rows.
HOLD_CASES = {"H25": ("H", 0.25), "H50": ("H", 0.5), "W50": ("W", 0.5)}
ALL_HELD = {"Hall": ("H", 0.75), "Wall": ("W", 0.75)}
HOLDS = dict(HOLD_CASES, **ALL_HELD)
IRLS_HOLDS = ("H25", "W50")

_CACHE = {}


def held_matrix(fraction, cv_seed=CV_SEED):
    key = ("held", fraction, cv_seed)
    if key not in _CACHE:
        _CACHE[key] = R.holdout(ROWS, COLS, fraction, cv_seed)
    return _CACHE[key]


def layout():
    """The designated rows and the dense column, chosen from the hash so that the hold-out conditions hold by construction."""
    if "layout" not in _CACHE:
        h25, h50 = held_matrix(0.25), held_matrix(0.5)
        dense_row = int(np.nonzero(h25[:, SINGLE_COL] & h25[:, ALLHELD_COL])[0][0])     # its entries of both columns are held out
        free = np.arange(FIRST_FREE, COLS)
        dense_col = int(free[np.argmax(h50[:, free].sum(axis=0))])
        taken = {dense_row}

        def pick(cond):
            r = next(int(r) for r in range(ROWS) if r not in taken and cond(r))
            taken.add(r)
            return r
        nheld = h50[:, free].sum(axis=1)
        lay = dict(dense_row=dense_row, dense_col=dense_col,
                   empty_rows=(pick(lambda r: True), pick(lambda r: r > 100)),
                   r1=pick(lambda r: h50[r, dense_col]),                   # W side: a single stored entry, held out
                   rall=pick(lambda r: h50[r, dense_col] and nheld[r] >= 5),   # W side: every stored entry held out
                   r32=pick(lambda r: nheld[r] >= 33), r33=pick(lambda r: nheld[r] >= 34), r31=pick(lambda r: nheld[r] >= 33))
        _CACHE["layout"] = lay
    return _CACHE["layout"]


def edge_matrix(kind="positive"):
    """131 x 67 CSC, rows sorted inside every column.  kind "positive": values in (0.5, 4) exact in float32 (MSE, Gamma, inverse
    Gaussian, Tweedie); "counts": integers 1..12 (GP, NB, MSE + robust).  Structure (a stored entry cannot lie in an empty row or
    column, so "dense" means every row or column that is not empty):
      column EMPTY_COL empty; rows layout()["empty_rows"] empty (empty columns of the W side);
      column layout()["dense_col"] stores every non-empty row (129), row layout()["dense_row"] every non-empty column (66);
      column SINGLE_COL: one stored entry, held out at 0.25 and 0.5; row "r1" the same on the W side;
      column ALLHELD_COL: six stored entries, all held out; row "rall" the same on the W side;
      columns C32, C33, C31 / rows "r32", "r33", "r31": exactly 32, 33, 31 held-out stored entries at fraction 0.5;
      column CAP_COL / row CAP_COL: an ordinary column whose start x is 0 (problem()): every IRLS weight of its first pass is capped."""
    key = ("A", kind)
    if key not in _CACHE:
        lay = layout()
        h25, h50 = held_matrix(0.25), held_matrix(0.5)
        rng = np.random.default_rng(MATRIX_SEED)
        S = rng.random((ROWS, COLS)) < 0.2
        drow, dcol = lay["dense_row"], lay["dense_col"]
        designed_rows = [lay[n] for n in ("r1", "rall", "r32", "r33", "r31")]
        pool = np.ones(ROWS, bool)
        pool[designed_rows + list(lay["empty_rows"]) + [drow]] = False
        free = np.arange(FIRST_FREE, COLS)
        free = free[free != dcol]
        S[:, [EMPTY_COL, SINGLE_COL, ALLHELD_COL, C32, C33, C31]] = False
        S[designed_rows, :] = False
        S[list(lay["empty_rows"]), :] = False
        S[:, dcol] = True
        S[list(lay["empty_rows"]), dcol] = False
        S[drow, :] = True
        S[drow, EMPTY_COL] = False
        for name, want, ntrain in (("r1", 1, 0), ("rall", 5, 0), ("r32", 32, 5), ("r33", 33, 5), ("r31", 31, 5)):
            r = lay[name]
            want -= int(h50[r, dcol])                                   # the dense column's entry counts
            S[r, free[h50[r, free]][:want]] = True
            S[r, free[~h50[r, free]][:ntrain]] = True
        rows = np.nonzero(pool)[0]
        S[rows[h25[rows, ALLHELD_COL]][:5], ALLHELD_COL] = True
        for c, want in ((C32, 32), (C33, 33), (C31, 31)):
            want -= int(h50[drow, c])
            S[rows[h50[rows, c]][:want], c] = True
            S[rows[~h50[rows, c]][:7], c] = True
        ri, ci = np.nonzero(S.T)[1], np.nonzero(S.T)[0]                 # column-major order, rows ascending inside a column
        p = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=COLS))])
        x = (rng.integers(1, 13, size=len(ri)).astype(np.float64) if kind == "counts"
             else rng.uniform(0.5, 4.0, size=len(ri)).astype(np.float32).astype(np.float64))
        _CACHE[key] = Pattern(ROWS, COLS, p, ri, x)
    return _CACHE[key]


def data(side, kind="positive"):
    """The CSC a half-update of `side` walks: A (H side) or its transpose (W side: 67 rows, 131 columns)."""
    key = ("D", side, kind)
    if key not in _CACHE:
        A = edge_matrix(kind)
        _CACHE[key] = A if side == "H" else A.transpose()
    return _CACHE[key]


def held_for(hold, cv_seed=CV_SEED):
    """(side, fraction, hold-out mask in the orientation of data(side))."""
    side, frac = HOLDS[hold]
    h = held_matrix(frac, cv_seed)
    return side, frac, (h if side == "H" else h.T)


def user_mask(side, empty=False):
    """The user mask of the runs of `side`, a pattern in the orientation of data(side) (the other orientation is its transpose):
    column 9 fully masked, columns 10..15 without an entry, 8 % of the entries of the other columns -- training nonzeros, training
    zeros, held-out nonzeros and held-out zeros among them (tests/test_cv_ref_cpu.py).  empty: no entry at all."""
    key = ("M", side, empty)
    if key not in _CACHE:
        D = data(side)
        rng = np.random.default_rng(900 + (side == "W"))
        U = rng.random((D.rows, D.cols)) < 0.08
        U[:, 9] = True
        U[:, 10:16] = False
        if empty:
            U[:] = False
        ci, ri = np.nonzero(U.T)
        p = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=D.cols))])
        _CACHE[key] = (Pattern(D.rows, D.cols, p, ri, np.ones(len(ri))), U)
    return _CACHE[key]


def problem(dtype, k, side):
    """(F, G, X0) of a side in `dtype`: F uniform(0.05, 1) with columns normalised to sum 30 (irls_inputs.factor),
    G = F^T F + RIDGE mean(diag) I of the rounded F; X0 uniform(0.05, 0.4) x 8 / k -- NOT zero: the CV solves start from the
    current column -- with row CAP_COL zero."""
    key = ("P", np.dtype(dtype), k, side)
    if key not in _CACHE:
        nrow, ncol = (ROWS, COLS) if side == "H" else (COLS, ROWS)
        rng = np.random.default_rng(300 + k + 1000 * (side == "W"))
        F = rng.uniform(0.05, 1.0, size=(nrow, k))
        F = (F / F.sum(axis=0, keepdims=True) * 30.0).astype(dtype)
        Fd = F.astype(np.float64)
        G = Fd.T @ Fd
        G[np.diag_indices(k)] += RIDGE * np.mean(np.diag(G))
        X0 = (rng.uniform(0.05, 0.4, size=(ncol, k)) * 8.0 / k).astype(dtype)
        X0[CAP_COL] = 0
        _CACHE[key] = (F, G.astype(dtype), X0)
    return _CACHE[key]


def g_add(dtype, k, solver, case):
    ridge = G_ADD_RIDGE["chol" if solver and LOSS_CASES[case][0] != 0 else "cd"]
    return (ridge * np.eye(k) + 0.01 * np.ones((k, k))).astype(dtype)


# MSE option cases: name -> keyword arguments of Context.solve_cv
MSE_BASE = dict(l1=0.01, nonneg=1, cd_maxit=20, solver_mode=0)
MSE_OPTIONS = {
    "cd": {},
    "cd_free": dict(nonneg=0),
    "cd_l1_0": dict(l1=0.0),
    "cd_1sweep": dict(cd_maxit=1),
    "chol": dict(solver_mode=1),
    "chol_free": dict(solver_mode=1, nonneg=0),
}
ALL_HELD_OPTIONS = dict(l1=0.01, nonneg=0, cd_maxit=3, solver_mode=0)      # b = 0: three sweeps still depend on G_local


def mse_options(opt):
    return ALL_HELD_OPTIONS if opt == "allheld" else dict(MSE_BASE, **MSE_OPTIONS[opt])


# IRLS loss cases: name -> (loss_type, power, robust, kind of matrix)
LOSS_CASES = {
    "gp": (4, 0.0, 0.0, "counts"),
    "nb": (5, 0.0, 0.0, "counts"),
    "gamma": (6, 0.0, 0.0, "positive"),
    "invgauss": (7, 0.0, 0.0, "positive"),
    "tweedie": (8, 1.6, 0.0, "positive"),
    "mse_robust": (0, 0.0, 1.345, "counts"),
    "gamma_robust": (6, 0.0, 1.345, "positive"),
}
# irls_tol = 0: `rel < 0` never holds, every column takes exactly irls_max_iter passes and no column is excused
IRLS_BASE = dict(l1=0.01, nonneg=1, cd_maxit=6, irls_max_iter=3, irls_tol=0.0)
# The early stop: one case of its own.  The statistic is a relative change PER COORDINATE, so a coordinate that leaves the clamp
# gives ~ 1e11 and six CD sweeps never settle it; MSE + robust with Cholesky on the W side does settle (the statistic's median falls
# from ~ 1e2 to ~ 0.2 over eight passes, the columns spread over two decades) and irls_tol = 0.7 stops columns at every pass from the
# third on.  A column is decisive when its statistic is outside irls_tol (1 +- margin) at every pass it ran: margin 1e-6 in fp64;
# 0.02 in fp32 -- the class's D (~ 1e-5 of max|ref|) moves a coordinate of 1e-3 of the largest by 1 % and the statistic by 2 %.
EARLY = dict(l1=0.01, nonneg=1, cd_maxit=6, irls_max_iter=8, irls_tol=0.7)
EARLY_CASE = ("mse_robust", "W50", 0, 1)                    # (loss case, hold, mask_zeros, solver)
EARLY_MARGIN = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 0.02}


def irls_options(case, solver, early=False):
    lt, power, robust, kind = LOSS_CASES[case]
    return dict(EARLY if early else IRLS_BASE, solver_mode=solver, loss_param=power, robust_delta=robust)


# Dispatch points: (dtype, k, mode, family).  mode "offset": F is a view one element into its buffer (4 bytes off for fp32, 8 for
# fp64: not 16-byte aligned), "mask": a user mask is set -- either keeps the MFMA kernels out.
f32, f64 = np.float32, np.float64
MSE_DISPATCH = (
    [(f32, k, "", "mfma32") for k in (4, 20, 32)] + [(f32, k, "", "mfma32x2") for k in (36, 64)]
    + [(f32, k, "", "reg32") for k in (1, 5, 31)] + [(f32, 32, "offset", "reg32"), (f32, 32, "mask", "reg32")]
    + [(f32, k, "", "reg64") for k in (33, 63)] + [(f32, 40, "offset", "reg64"), (f32, 64, "mask", "reg64")]
    + [(f32, k, "", "wide") for k in (65, 100, 128)] + [(f32, k, "mask", "wide") for k in (65, 128)]
    + [(f64, k, "", "mfma64") for k in (2, 18, 32)]
    + [(f64, k, "", "reg32") for k in (1, 31)] + [(f64, 32, "offset", "reg32"), (f64, 32, "mask", "reg32")]
    + [(f64, k, "", "reg64") for k in (33, 64)] + [(f64, 64, "mask", "reg64")]
    + [(f64, k, "", "wide") for k in (65, 100, 128)] + [(f64, k, "mask", "wide") for k in (65, 128)])
IRLS_DISPATCH = [(dt, k, "", fam) for dt in (f32, f64) for fam, ks in (("reg32", (6, 32)), ("reg64", (33, 64)), ("wide", (65, 128)))
                 for k in ks]
LOSS_KS = (1, 63, 64, 65, 128)          # cv_test_error_kernel / cv_irls_loss_kernel: the second feature per lane starts at k = 65


def kernel_reached(dtype, k, aligned, masked):
    """The instantiation cv_solve_impl (ops_cv.hip) launches, restated from its conditions (RCPPML_GPU_CV_VARIANT unset)."""
    T = "float" if np.dtype(dtype) == np.float32 else "double"
    if k > 64:
        return "wide_cv_solve_kernel<%s>" % T
    if T == "float" and not masked and aligned and k % 4 == 0:
        return "cv_solve_mfma32_kernel" if k <= 32 else "cv_solve_mfma32x2_kernel"
    if T == "double" and not masked and aligned and k <= 32 and k % 2 == 0:
        return "cv_solve_mfma64_kernel"
    return "cv_solve_kernel<%s,%d>" % (T, 32 if k <= 32 else 64)


def irls_kernel_reached(dtype, k):
    """The instantiation solve_impl of ops_cv_irls.hip.h launches."""
    T = "float" if np.dtype(dtype) == np.float32 else "double"
    return "wide_cv_irls_solve_kernel<%s>" % T if k > 64 else "cv_irls_solve_kernel<%s,%d>" % (T, 32 if k <= 32 else 64)


FAMILY_KERNEL = {"mfma32": "cv_solve_mfma32_kernel", "mfma32x2": "cv_solve_mfma32x2_kernel", "mfma64": "cv_solve_mfma64_kernel",
                 "reg32": "cv_solve_kernel<%s,32>", "reg64": "cv_solve_kernel<%s,64>", "wide": "wide_cv_solve_kernel<%s>"}
IRLS_FAMILY_KERNEL = {"reg32": "cv_irls_solve_kernel<%s,32>", "reg64": "cv_irls_solve_kernel<%s,64>", "wide": "wide_cv_irls_solve_kernel<%s>"}


def point_id(pt):
    dtype, k, mode, fam = pt
    return "%s-k%d-%s%s" % (np.dtype(dtype).name, k, fam, "-" + mode if mode else "")


# ---------------------------------------------------------------------------------------------------------------------------
# References (float64 restatement of the dtype-rounded inputs; xp = numpy.longdouble for the fp64 bounds)
# ---------------------------------------------------------------------------------------------------------------------------
def mse_reference(dtype, k, hold, mask_zeros, opt, masked=False, xp=np.float64, cv_seed=CV_SEED):
    key = ("Rm", np.dtype(dtype), k, hold, mask_zeros, opt, masked, np.dtype(xp), cv_seed)
    if key not in _CACHE:
        side, frac, held = held_for(hold, cv_seed)
        F, G, X0 = problem(dtype, k, side)
        kw = mse_options(opt)
        _CACHE[key] = R.mse_half_update(data(side), F, G, X0, held, mask_zeros=bool(mask_zeros), umask=user_mask(side)[1] if masked else None,
                                        l1=q(kw["l1"], dtype), nonneg=bool(kw["nonneg"]), cd_maxit=kw["cd_maxit"],
                                        solver_mode=kw["solver_mode"], xp=xp)
    return _CACHE[key]


def irls_reference(dtype, k, case, hold, mask_zeros, solver, masked=False, early=False, xp=np.float64):
    """(X, passes, stat, trace)."""
    key = ("Ri", np.dtype(dtype), k, case, hold, mask_zeros, solver, masked, early, np.dtype(xp))
    if key not in _CACHE:
        side, frac, held = held_for(hold)
        lt, power, robust, kind = LOSS_CASES[case]
        F, G, X0 = problem(dtype, k, side)
        Ga = g_add(dtype, k, solver, case)
        kw = irls_options(case, solver, early)
        trace = {}
        out = R.irls_half_update(data(side, kind), F, Ga, X0, held, mask_zeros=bool(mask_zeros), loss_type=lt, dtype=dtype,
                                 umask=user_mask(side)[1] if masked else None, l1=q(kw["l1"], dtype), nonneg=bool(kw["nonneg"]),
                                 cd_maxit=kw["cd_maxit"], solver_mode=solver, irls_max_iter=kw["irls_max_iter"],
                                 irls_tol=q(kw["irls_tol"], dtype), power=q(power, dtype), robust=q(robust, dtype), xp=xp, trace=trace)
        _CACHE[key] = out + (trace,)
    return _CACHE[key]


def decisive_columns(dtype, k):
    """The early-stop case: columns whose stop statistic lies outside irls_tol (1 +- EARLY_MARGIN) at every pass they ran --
    computed from the restatement alone."""
    from tests.cd_ref import decisive
    case, hold, mz, solver = EARLY_CASE
    stat = irls_reference(dtype, k, case, hold, mz, solver, early=True)[2]
    return decisive(stat, q(EARLY["irls_tol"], dtype), EARLY_MARGIN[np.dtype(dtype)])


def loss_problem(dtype, k):
    """(W, d, H, theta) of the loss kernels on the edge matrix."""
    key = ("L", np.dtype(dtype), k)
    if key not in _CACHE:
        rng = np.random.default_rng(50 + k)
        W = (rng.uniform(0.1, 1.0, size=(ROWS, k)) / np.sqrt(k)).astype(dtype)
        H = (rng.uniform(0.1, 1.0, size=(COLS, k)) / np.sqrt(k)).astype(dtype)
        d = rng.uniform(0.5, 2.0, size=k).astype(dtype)
        theta = rng.uniform(0.0, 0.8, size=ROWS).astype(dtype)
        _CACHE[key] = (W, d, H, theta)
    return _CACHE[key]


LOSS_TYPES = {0: ("counts", 0.0), 4: ("counts", 0.0), 5: ("counts", 0.0), 6: ("positive", 0.0), 7: ("positive", 0.0), 8: ("positive", 1.4)}
LOSS_HOLD = 0.25


def loss_reference(dtype, k, loss_type, mask_zeros, masked=False, xp=np.float64):
    key = ("Rl", np.dtype(dtype), k, loss_type, mask_zeros, masked, np.dtype(xp))
    if key not in _CACHE:
        W, d, H, theta = loss_problem(dtype, k)
        kind, power = LOSS_TYPES[loss_type]
        _CACHE[key] = R.explicit_loss(edge_matrix(kind), W, d, H, held_matrix(LOSS_HOLD), mask_zeros=bool(mask_zeros), loss_type=loss_type,
                                      dtype=dtype, theta=theta, power=power, umask=user_mask("H")[1] if masked else None, xp=xp)
    return _CACHE[key]


def error_reference(dtype, k, mask_zeros, xp=np.float64):
    key = ("Re", np.dtype(dtype), k, mask_zeros, np.dtype(xp))
    if key not in _CACHE:
        W, d, H, theta = loss_problem(dtype, k)
        _CACHE[key] = R.heldout_error(edge_matrix("positive"), W, d, H, held_matrix(LOSS_HOLD), mask_zeros=bool(mask_zeros), dtype=dtype, xp=xp)
    return _CACHE[key]


def deviation(X, Xr):
    """max|X - Xr| / max|Xr|."""
    Xr = np.asarray(Xr, np.float64)
    return float(np.abs(np.asarray(X, np.float64) - Xr).max() / max(np.abs(Xr).max(), 1e-300))


# ---------------------------------------------------------------------------------------------------------------------------
# Bounds, relative to max|ref|.  Nothing measured on a GPU sets one.
# fp32: 4 x D rounded up to one digit, D = the worst deviation of the fp32 ORACLE from the float64 restatement on the same
#   fp32-rounded inputs over the class, measured on the CPU (tests/test_cv_ref_cpu.py prints D and asserts D <= bound / 4) -- the
#   project's rule (cd_inputs.py, irls_inputs.py): a correct fp32 kernel with another summation order gets the room the oracle's
#   own rounding takes.  Classes: MSE (k class, solver or "allheld"); IRLS (k class, solver, loss case); the loss kernels (loss).
# fp64: 4 x the fp64 oracle's deviation from the restatement evaluated in numpy.longdouble (FP64_D, measured at FP64_KS), floored
#   at 1e-12 and never above what tests/test_gpu_cv.py allows (1e-8 MSE, 1e-7 IRLS, 1e-11 the sums).
# ---------------------------------------------------------------------------------------------------------------------------
def k_class(k):
    return "k<=32" if k <= 32 else ("k<=64" if k <= 64 else "wide")


# class: D (the measured value rounded up in its third digit),  # where it is reached: (k, hold-out case, mask_zeros, ...)
FP32_D = {
    ('irls', 'k<=32', 'cd', 'gamma'): 2.12e-06,                # (32, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'gamma_robust'): 1.25e-06,         # (32, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'gp'): 1.81e-06,                   # (32, 'H25', 1)
    ('irls', 'k<=32', 'cd', 'invgauss'): 2.37e-06,             # (32, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'mse_robust'): 2.16e-06,           # (32, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'nb'): 2.79e-06,                   # (32, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'tweedie'): 1.84e-06,              # (32, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'gamma'): 1.64e-05,              # (32, 'W50', 0)
    ('irls', 'k<=32', 'chol', 'gamma_robust'): 4.03e-06,       # (32, 'W50', 0)
    ('irls', 'k<=32', 'chol', 'gp'): 4.44e-06,                 # (32, 'W50', 0)
    ('irls', 'k<=32', 'chol', 'invgauss'): 1.64e-05,           # (32, 'W50', 0)
    ('irls', 'k<=32', 'chol', 'mse_robust'): 5.31e-06,         # (32, 'H25', 1)
    ('irls', 'k<=32', 'chol', 'nb'): 8.44e-06,                 # (32, 'W50', 0)
    ('irls', 'k<=32', 'chol', 'tweedie'): 1.64e-05,            # (32, 'W50', 0)
    ('irls', 'k<=64', 'cd', 'gamma'): 2.42e-06,                # (64, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'gamma_robust'): 3.22e-06,         # (64, 'H25', 1)
    ('irls', 'k<=64', 'cd', 'gp'): 2.27e-06,                   # (33, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'invgauss'): 3.07e-06,             # (64, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'mse_robust'): 2.15e-06,           # (64, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'nb'): 3.47e-06,                   # (64, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'tweedie'): 2.10e-06,              # (33, 'H25', 0)
    ('irls', 'k<=64', 'chol', 'gamma'): 4.76e-05,              # (64, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'gamma_robust'): 5.34e-06,       # (33, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'gp'): 5.51e-06,                 # (64, 'H25', 0)
    ('irls', 'k<=64', 'chol', 'invgauss'): 4.76e-05,           # (64, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'mse_robust'): 9.76e-06,         # (33, 'H25', 0)
    ('irls', 'k<=64', 'chol', 'nb'): 4.23e-05,                 # (64, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'tweedie'): 4.76e-05,            # (64, 'W50', 0)
    ('irls', 'wide', 'cd', 'gamma'): 3.20e-06,                 # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'gamma_robust'): 2.54e-06,          # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'gp'): 3.52e-06,                    # (128, 'H25', 0)
    ('irls', 'wide', 'cd', 'invgauss'): 2.06e-06,              # (128, 'H25', 1)
    ('irls', 'wide', 'cd', 'mse_robust'): 3.81e-06,            # (65, 'H25', 1)
    ('irls', 'wide', 'cd', 'nb'): 3.61e-06,                    # (128, 'H25', 1)
    ('irls', 'wide', 'cd', 'tweedie'): 2.56e-06,               # (128, 'H25', 0)
    ('irls', 'wide', 'chol', 'gamma'): 6.19e-05,               # (128, 'W50', 1)
    ('irls', 'wide', 'chol', 'gamma_robust'): 3.09e-06,        # (128, 'H25', 0)
    ('irls', 'wide', 'chol', 'gp'): 1.49e-05,                  # (128, 'H25', 0)
    ('irls', 'wide', 'chol', 'invgauss'): 6.19e-05,            # (128, 'W50', 1)
    ('irls', 'wide', 'chol', 'mse_robust'): 9.44e-06,          # (128, 'W50', 1)
    ('irls', 'wide', 'chol', 'nb'): 4.58e-05,                  # (128, 'W50', 0)
    ('irls', 'wide', 'chol', 'tweedie'): 4.67e-05,             # (128, 'H25', 0)
    ('mse', 'k<=32', 'allheld'): 9.88e-07,                     # (31, 'Hall', 0, 'allheld', False)
    ('mse', 'k<=32', 'cd'): 5.58e-06,                          # (20, 'H25', 1, 'cd_l1_0', False)
    ('mse', 'k<=32', 'chol'): 6.25e-06,                        # (31, 'H25', 1, 'chol', False)
    ('mse', 'k<=64', 'allheld'): 2.79e-06,                     # (64, 'Hall', 0, 'allheld', False)
    ('mse', 'k<=64', 'cd'): 7.01e-06,                          # (63, 'H50', 1, 'cd_l1_0', False)
    ('mse', 'k<=64', 'chol'): 6.43e-06,                        # (63, 'H25', 0, 'chol', False)
    ('mse', 'wide', 'allheld'): 1.32e-05,                      # (128, 'Hall', 0, 'allheld', False)
    ('mse', 'wide', 'cd'): 7.35e-06,                           # (128, 'H25', 1, 'cd_free', True)
    ('mse', 'wide', 'chol'): 7.47e-06,                         # (128, 'H25', 1, 'chol_free', False)
    ('sum', 'error'): 1.27e-06,                                # (1, 0)
    ('sum', 0): 1.77e-06,                                      # (128, 0, False)
    ('sum', 4): 2.65e-06,                                      # (64, 0, False)
    ('sum', 5): 2.98e-06,                                      # (1, 0, False)
    ('sum', 6): 3.87e-06,                                      # (63, 0, True)
    ('sum', 7): 4.89e-05,                                      # (1, 0, False)
    ('sum', 8): 2.42e-06,                                      # (128, 0, False)
}
FP64_D = {
    ('irls', 'k<=32', 'cd', 'gamma'): 2.51e-15,                # (6, 'H25', 0, 'masked')
    ('irls', 'k<=32', 'cd', 'gamma_robust'): 1.77e-15,         # (6, 'H25', 1)
    ('irls', 'k<=32', 'cd', 'gp'): 1.98e-15,                   # (6, 'H25', 0)
    ('irls', 'k<=32', 'cd', 'invgauss'): 2.08e-15,             # (6, 'H25', 1)
    ('irls', 'k<=32', 'cd', 'mse_robust'): 1.23e-15,           # (6, 'H25', 1)
    ('irls', 'k<=32', 'cd', 'nb'): 2.55e-15,                   # (6, 'H25', 1)
    ('irls', 'k<=32', 'cd', 'tweedie'): 2.45e-15,              # (6, 'H25', 1)
    ('irls', 'k<=32', 'chol', 'gamma'): 2.66e-15,              # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'gamma_robust'): 3.25e-15,       # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'gp'): 9.91e-16,                 # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'invgauss'): 2.66e-15,           # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'mse_robust'): 5.70e-15,         # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'nb'): 2.01e-15,                 # (6, 'H25', 0)
    ('irls', 'k<=32', 'chol', 'tweedie'): 2.95e-15,            # (6, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'gamma'): 5.07e-15,                # (33, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'gamma_robust'): 3.00e-15,         # (33, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'gp'): 2.89e-15,                   # (33, 'H25', 1)
    ('irls', 'k<=64', 'cd', 'invgauss'): 3.77e-15,             # (33, 'H25', 1)
    ('irls', 'k<=64', 'cd', 'mse_robust'): 3.98e-15,           # (33, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'nb'): 3.36e-15,                   # (33, 'H25', 0)
    ('irls', 'k<=64', 'cd', 'tweedie'): 3.56e-15,              # (33, 'H25', 1)
    ('irls', 'k<=64', 'chol', 'gamma'): 3.56e-14,              # (33, 'W50', 1)
    ('irls', 'k<=64', 'chol', 'gamma_robust'): 1.30e-14,       # (33, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'gp'): 1.10e-14,                 # (33, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'invgauss'): 3.56e-14,           # (33, 'W50', 1)
    ('irls', 'k<=64', 'chol', 'mse_robust'): 1.72e-14,         # (33, 'H25', 0)
    ('irls', 'k<=64', 'chol', 'nb'): 1.86e-14,                 # (33, 'W50', 0)
    ('irls', 'k<=64', 'chol', 'tweedie'): 3.56e-14,            # (33, 'W50', 1)
    ('irls', 'wide', 'cd', 'gamma'): 3.66e-15,                 # (65, 'H25', 1)
    ('irls', 'wide', 'cd', 'gamma_robust'): 5.53e-15,          # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'gp'): 5.96e-15,                    # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'invgauss'): 5.59e-15,              # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'mse_robust'): 5.76e-15,            # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'nb'): 2.41e-15,                    # (65, 'H25', 0)
    ('irls', 'wide', 'cd', 'tweedie'): 4.43e-15,               # (65, 'H25', 1)
    ('irls', 'wide', 'chol', 'gamma'): 6.45e-14,               # (65, 'W50', 0)
    ('irls', 'wide', 'chol', 'gamma_robust'): 4.28e-15,        # (65, 'H25', 0)
    ('irls', 'wide', 'chol', 'gp'): 1.07e-14,                  # (65, 'H25', 0)
    ('irls', 'wide', 'chol', 'invgauss'): 6.45e-14,            # (65, 'W50', 0)
    ('irls', 'wide', 'chol', 'mse_robust'): 2.06e-14,          # (65, 'H25', 1)
    ('irls', 'wide', 'chol', 'nb'): 5.09e-14,                  # (65, 'W50', 0)
    ('irls', 'wide', 'chol', 'tweedie'): 6.45e-14,             # (65, 'W50', 0)
    ('mse', 'k<=32', 'allheld'): 6.63e-16,                     # (18, 'Hall', 0, 'allheld', False)
    ('mse', 'k<=32', 'cd'): 5.33e-15,                          # (18, 'H25', 0, 'cd_free', False)
    ('mse', 'k<=32', 'chol'): 5.59e-15,                        # (18, 'H25', 1, 'chol', False)
    ('mse', 'k<=64', 'allheld'): 1.29e-15,                     # (33, 'Hall', 0, 'allheld', False)
    ('mse', 'k<=64', 'cd'): 1.07e-14,                          # (33, 'H25', 0, 'cd_l1_0', False)
    ('mse', 'k<=64', 'chol'): 8.76e-15,                        # (33, 'H25', 1, 'chol', False)
    ('mse', 'wide', 'allheld'): 5.49e-15,                      # (65, 'Hall', 0, 'allheld', False)
    ('mse', 'wide', 'cd'): 1.89e-14,                           # (65, 'H25', 1, 'cd', False)
    ('mse', 'wide', 'chol'): 1.35e-14,                         # (65, 'H25', 1, 'chol', False)
    ('sum', 'error'): 1.57e-15,                                # (65, 1)
    ('sum', 0): 2.62e-15,                                      # (65, 1, False)
    ('sum', 4): 3.71e-15,                                      # (65, 0, True)
    ('sum', 5): 3.37e-15,                                      # (1, 1, True)
    ('sum', 6): 2.88e-15,                                      # (1, 0, True)
    ('sum', 7): 3.48e-15,                                      # (65, 0, True)
    ('sum', 8): 3.19e-15,                                      # (65, 0, True)
}
FP64_KS = (2, 18, 33, 65)
FP64_IRLS_KS = (6, 33, 65)
FP64_CHECK_KS = ((2, 33), (6,))      # (MSE, IRLS): what tests/test_cv_ref_cpu.py measures again on every run
FP64_CAP = {"mse": 1e-8, "irls": 1e-7, "sum": 1e-11}


def bound(dtype, cls):
    """cls: ("mse", k class, "cd" / "chol" / "allheld"), ("irls", k class, solver, loss case), ("sum", "error" / loss type)."""
    if np.dtype(dtype) == np.float32:
        return round_up_1(4 * FP32_D[cls])
    return min(max(round_up_1(4 * FP64_D[cls]), 1e-12), FP64_CAP[cls[0]])


def mse_class(k, opt):
    return ("mse", k_class(k), "allheld" if opt == "allheld" else ("chol" if mse_options(opt)["solver_mode"] else "cd"))


def irls_class(k, solver, case):
    return ("irls", k_class(k), "chol" if solver else "cd", case)
