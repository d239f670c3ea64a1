"""Shared inputs of tests/test_irls_ref_cpu.py and tests/test_gpu_irls_matrix.py: the edge matrix, the factor matrix and its Gram,
the loss and option cases, the dispatch points of rcppml_hip_solve_irls, the bounds and the float64 references of
tests/irls_ref.py, computed once per process and shared.  numpy only: no torch, no GPU code, no oracle."""
import numpy as np

from tests.cd_inputs import Pattern, q
from tests.irls_ref import irls_half_update

ROWS, COLS = 97, 67                 # ragged for the 4-column blocks and for the quad kernel's 16-column blocks
# stored entries of the first columns: the chunk edges of every kernel (32: mfma32 / x2 / mfma64, 64: mfma32q, 8: wide), the MFMA
# steps (two nonzeros in fp32, four in fp64), the empty column and the dense one
EDGE_COUNTS = (0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 97)
OUTLIER = (40, 20)                  # (row, column) of the entry about 1e3 times the typical one (a random column, 5..40 entries)
MATRIX_SEED = 11
# kind "dense": F's seed is shifted by 100000 x this at the k where the first seed left more than 5 % of the columns of an early-stop
# case non-decisive in fp32 (k = 31: 4 of 67 for nb_early; k = 36: 4 for gp_early, then 4 for nb_early; k = 3: 4 for gp_early)
DENSE_F_SHIFT = {3: 1, 31: 1, 36: 2}
# kind "dense" (the NB / GP early stop, see EARLY_CASES): stored entries of the random columns, largest count, ridge; no outlier
DENSE_COUNTS, DENSE_MAX, RIDGE_DENSE = (60, 97), 3, 1e-3
F_SEED = 100                        # + k
RIDGE = 0.25    # on the base Gram, a fraction of its mean diagonal (masked_gram): see BOUNDS below


def edge_matrix(kind):
    """97 x 67 CSC, rows sorted inside every column.  kind "counts": integer counts 1..12 (NB, GP, MSE); "positive": strictly
    positive continuous values in (0.05, 4) (Gamma, inverse Gaussian, Tweedie).  Entry OUTLIER is about 1e3 times the typical one.
    kind "dense" (the converging early-stop cases, EARLY_CASES): the same edge columns, every other column with DENSE_COUNTS stored
    entries, integer counts 1..DENSE_MAX, no outlier."""
    key = ("A", kind)
    if key not in _CACHE:
        rng = np.random.default_rng(MATRIX_SEED)
        p, ri, xv = [0], [], []
        for j in range(COLS):
            cnt = EDGE_COUNTS[j] if j < len(EDGE_COUNTS) else int(rng.integers(5, 41))
            if kind == "dense" and j >= len(EDGE_COUNTS):
                cnt = int(rng.integers(DENSE_COUNTS[0], DENSE_COUNTS[1] + 1))
            r = np.sort(rng.choice(ROWS, size=cnt, replace=False))
            if kind != "dense" and j == OUTLIER[1] and OUTLIER[0] not in r:
                r[np.searchsorted(r, OUTLIER[0]) % cnt] = OUTLIER[0]
                r = np.sort(np.unique(r))
                cnt = len(r)
            cvals = rng.integers(1, 13, size=cnt).astype(np.float64)
            pvals = rng.uniform(0.05, 4.0, size=cnt).astype(np.float32).astype(np.float64)     # exact in both dtypes
            v = cvals if kind == "counts" else pvals
            if kind == "dense":
                v = rng.integers(1, DENSE_MAX + 1, size=cnt).astype(np.float64)
            elif j == OUTLIER[1]:
                v[np.nonzero(r == OUTLIER[0])[0][0]] = 5000.0 if kind == "counts" else 2000.0
            ri.append(r); xv.append(v); p.append(p[-1] + cnt)
        _CACHE[key] = Pattern(ROWS, COLS, p, np.concatenate(ri), np.concatenate(xv))
    return _CACHE[key]


def factor(rows, k, dtype, ridge=None, shift=0):
    """F as in tests/test_gpu_nb.py (uniform(0.05, 1), columns normalised to sum 30), rounded to dtype, and
    G = F^T F + RIDGE * mean(diag) * I of the rounded F, rounded to dtype (cd_inputs.masked_gram)."""
    rng = np.random.default_rng(F_SEED + k + 1000 * rows + 100000 * shift)
    F = rng.uniform(0.05, 1.0, size=(rows, k))
    F /= F.sum(axis=0, keepdims=True)
    F = (F * 30.0).astype(dtype)
    Fd = F.astype(np.float64)
    G = Fd.T @ Fd
    G[np.diag_indices(k)] += (RIDGE if ridge is None else ridge) * np.mean(np.diag(G))
    return F, G.astype(dtype)


# Loss cases: name -> (loss_type, theta ("row" / "col" / None), power, robust, kind of matrix).  theta by column runs on the
# TRANSPOSED edge matrix (67 x 97: 97 columns, F has 67 rows), as the W side of a fit does.
LOSS_CASES = {
    "nb_row": (5, "row", 0.0, 0.0, "counts"),
    "nb_col": (5, "col", 0.0, 0.0, "counts"),
    "nb_none": (5, None, 0.0, 0.0, "counts"),
    "gp": (4, None, 0.0, 0.0, "counts"),
    "gamma": (6, None, 0.0, 0.0, "positive"),
    "invgauss": (7, None, 0.0, 0.0, "positive"),
    "tweedie": (8, None, 1.5, 0.0, "positive"),
    "mse_robust": (0, None, 0.0, 1.345, "counts"),
    "nb_robust": (5, "row", 0.0, 1.345, "counts"),
    "gamma_robust": (6, None, 0.0, 1.345, "positive"),
}
EARLY_LOSS_CASES = {"nb_early": (5, "row", 0.0, 0.0, "dense"), "gp_early": (4, None, 0.0, 0.0, "dense"),
                    "mse_early": (0, None, 0.0, 1.345, "dense")}
MATRIX_LOSSES = tuple(LOSS_CASES)
LOSS_CASES.update(EARLY_LOSS_CASES)
FAMILY = {"nb_row": "nb", "nb_col": "nb", "nb_none": "nb", "gp": "gp", "gamma": "power", "invgauss": "power", "tweedie": "power",
          "mse_robust": "robust", "nb_robust": "robust", "gamma_robust": "robust", "nb_early": "nb", "gp_early": "gp", "mse_early": "robust"}
# Option cases: name -> what changes against BASE.  cd_maxit is short (8) through the matrix -- the float64 restatement costs
# cd_maxit x k numpy steps per pass -- and "cd100" is the reference's default of 100 sweeps, once per kernel.
BASE = dict(l1=0.0, l2=1e-3, nonneg=1, cd_maxit=8, irls_max_iter=4, irls_tol=0.0)
OPTION_CASES = {
    "base": {},
    "l1": dict(l1=0.05),
    "free": dict(nonneg=0),
    "l1_free": dict(l1=0.02, nonneg=0),
    "l2_0": dict(l2=0.0),
    "cd3": dict(cd_maxit=3),
    "iter1": dict(irls_max_iter=1),
    "iter2": dict(irls_max_iter=2),
    "tol0": dict(irls_max_iter=6),                       # irls_tol = 0: rel < 0 never holds, all six passes run
    "early": dict(irls_max_iter=8, irls_tol=1e-4),
    "early2": dict(irls_max_iter=8, irls_tol=1e-1),
    "early3": dict(irls_max_iter=10, irls_tol=1e-1, cd_maxit=30, l2=0.0),
    "cd100": dict(cd_maxit=100, irls_max_iter=2),
}
# NB without theta takes r = max(0, 1e-10): from the second pass on the weights are ~ 1e-10 / mu^2 and the iterate drops from O(1)
# to ~ 1e-10 by cancellation (b = sum f w a - G_w x_old with x_old of O(1)): relative to max|ref| ~ 1e-10 the float64 oracle
# and the float64 restatement themselves agree to 1e-3 only, the fp32 oracle not at all.  So the case runs ONE pass from x = 0,
# in which every weight sits at the 1e6 cap whatever theta is (the restatement with any theta_row gives the same result exactly):
# the case proves that a null theta pointer is handled and the column solved, not that r = max(0, 1e-10) is computed right -- a
# kernel that took a wrong theta here would pass.  theta itself is pinned by nb_row, nb_col and nb_robust.
LOSS_OVERRIDES = {"nb_none": dict(irls_max_iter=1)}
OPTION_LOSSES = ("nb_row", "gp")
# Early stop.  On the edge matrix the NB and GP iterations do not settle: where the unweighted part of G_w (the rows without a
# stored entry, weight 1, and the ridge) outweighs the weighted one, a pass maps x to ~ 1 / x_old in that direction and the
# iterate oscillates with a factor ~ 0.9 per pass (40 passes do not bring the statistic of most columns below 1e-2, whatever
# cd_maxit), and a clamped coordinate that leaves 0 gives a statistic ~ 1e12.  "early" (irls_tol = 1e-4, the reference's default)
# therefore stops the empty column and one or two others only: it stays in the matrix and holds the kernels to "no stop" at
# that tolerance.  The cases in which columns DO stop, at several pass counts (CONVERGING):
#   nb_early, gp_early / "early3": the matrix of kind "dense" (the edge columns, then 60 to 97 stored entries, counts 1..3, no
#     outlier) with a ridge of 1e-3 and l2 = 0, so that the weighted part carries G_w; 30 sweeps, 10 passes, irls_tol = 0.1.
#   mse_early / "early2": MSE + robust on the same matrix, Huber weights, a factor ~ 4.5 per pass; irls_tol = 0.1, 8 passes.
# Why 0.1 and not 1e-4: the statistic max_i |x_i - x_old_i| / (|x_old_i| + 1e-12) is a relative change PER COORDINATE.  An absolute
# error e of the iterate moves it by ~ 2 e / |x_i|; with e = 2e-5 of the column's largest entry (EARLY_NOISE) that is 1e-4 for every
# coordinate below 40 % of the largest -- no fp32 computation, the fp32 oracle included, decides a stop at 1e-4 or 1e-2 on more than
# a part of the columns (measured: 30 to 95 % non-decisive).  At 0.1 at most 3 of 67 columns are non-decisive at every k.
EARLY_CASES = (("nb_row", "early"), ("gp", "early"), ("nb_early", "early3"), ("gp_early", "early3"), ("mse_early", "early2"))
CONVERGING = EARLY_CASES[2:]
EARLY_DELTA = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-2}
# fp32: absolute error allowed for in an iterate when a pass's stop is judged decisive, as a fraction of the COLUMN's largest
# entry: the robust class's D (the fp32 oracle's own deviation) of FP32_D, rounded up.  (The fp32 oracle's worst column on the
# converging cases is 7e-6 for MSE + robust and 2e-5 to 3.5e-5 for NB and GP; what holds the rule to account is that on the columns
# it calls decisive the fp32 oracle's pass counts equal the restatement's: test_irls_ref_cpu.py.)
EARLY_NOISE = {np.dtype(np.float64): 0.0, np.dtype(np.float32): 2e-5}

# Dispatch points of irls_impl (rcppml_amd/csrc/ops_irls.hip): (dtype, k, mode, kernel).  mode "cpw1" / "cpw4": OPT_IRLS_COLUMNS_PER_WAVE
# forced to 1 / 4 (67 columns are far below the 64 x CUs at which the quad kernel is taken by itself); "offset": F is a view
# that starts one element into its buffer, so it is not 16-byte aligned and the MFMA kernels are not taken.  NB without the robust
# modifier reaches the <5> instantiation of mfma32 / mfma32q, every other loss case <-1>.
DISPATCH = (
    [(np.float32, k, "cpw1", "mfma32") for k in (4, 16, 32)] + [(np.float32, k, "cpw4", "mfma32q") for k in (4, 16, 32)]
    + [(np.float32, k, "", "mfma32x2") for k in (36, 48, 64)] + [(np.float32, k, "", "reg32") for k in (5, 31)]
    + [(np.float32, k, "", "reg64") for k in (33, 62)] + [(np.float32, k, "", "wide") for k in (65, 96, 128)]
    + [(np.float32, 16, "offset", "reg32"), (np.float32, 48, "offset", "reg64")]
    + [(np.float64, k, "", "mfma64") for k in (2, 16, 32)] + [(np.float64, k, "", "reg32") for k in (3, 31)]
    + [(np.float64, k, "", "reg64") for k in (33, 64)] + [(np.float64, k, "", "wide") for k in (65, 128)]
    + [(np.float64, 16, "offset", "reg32")])


def kernel_reached(dtype, k, mode, loss_type, robust):
    """The instantiation irls_impl launches, restated from its conditions (the RCPPML_GPU_IRLS_VARIANT experiment variable unset)."""
    f32 = np.dtype(dtype) == np.float32
    T = "float" if f32 else "double"
    aligned = mode != "offset"
    if k > 64:
        return "wide_irls_solve_kernel<%s>" % T
    if f32 and k <= 32 and k % 4 == 0 and aligned:
        lt = "<5>" if loss_type == 5 and not robust > 0 else "<-1>"
        assert mode in ("cpw1", "cpw4")
        return ("irls_nb_mfma32q_kernel" if mode == "cpw4" else "irls_nb_mfma32_kernel") + lt
    if f32 and k % 4 == 0 and aligned:
        return "irls_nb_mfma32x2_kernel"
    if not f32 and k <= 32 and k % 2 == 0 and aligned:
        return "irls_nb_mfma64_kernel"
    return "irls_nb_solve_kernel<%s,%d>" % (T, 32 if k <= 32 else 64)


def point_id(pt):
    dtype, k, mode, kern = pt
    return "%s-k%d-%s%s" % (np.dtype(dtype).name, k, kern, "-" + mode if mode else "")


def round_up_1(v):
    """v rounded up to one significant digit."""
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10 ** e * (1 - 1e-12)) * 10 ** e)


# Bounds, relative to max|ref|.  fp64: the project's existing 1e-7 (NB, GP) and 1e-6 (power family, robust).  fp32: 4 x D rounded up
# to one significant digit, D = the worst deviation of the fp32 ORACLE from the float64 restatement on the same fp32-rounded inputs,
# over the class (family x clamped / unclamped x k <= 64 / k > 64), every loss and option case and every k of DISPATCH, measured
# on the CPU (tests/test_irls_ref_cpu.py::test_fp32_bounds prints and asserts D <= bound / 4).  The factor 4 is the margin
# cd_inputs.py uses: a correct fp32 kernel with another summation order gets the room the oracle's own rounding takes.
# The early-stop cases enter with their decisive columns, the unclamped ones with their kept columns.
# (D with the outlier's column, D without it); where the first is far larger, it is the outlier's column alone that sets it.
FP32_D = {
    ("gp", "clamped", "k<=64"): (6.41e-3, 1.67e-4),      # gp/cd3 at k = 36: 6.4e-3, every other case <= 7.8e-4
    ("gp", "clamped", "wide"): (8.29e-4, 1.99e-5),
    ("gp", "free", "k<=64"): (1.51e-4, 2.18e-4),
    ("gp", "free", "wide"): (2.31e-4, 2.31e-4),
    ("nb", "clamped", "k<=64"): (8.53e-4, 2.53e-5),
    ("nb", "clamped", "wide"): (9.50e-4, 2.57e-5),
    ("nb", "free", "k<=64"): (6.95e-4, 6.95e-4),
    ("nb", "free", "wide"): (2.31e-4, 2.31e-4),
    ("power", "clamped", "k<=64"): (3.18e-4, 2.17e-5),
    ("power", "clamped", "wide"): (4.12e-4, 1.91e-5),
    ("robust", "clamped", "k<=64"): (1.39e-5, 1.39e-5),
    ("robust", "clamped", "wide"): (1.13e-5, 1.13e-5),     # mse_early/early2 at k = 128; the loss cases alone 9.13e-6
}
FP32_BOUND = {c: (round_up_1(4 * d[0]), round_up_1(4 * d[1])) for c, d in FP32_D.items()}


def bound(dtype, case, nonneg, k):
    """(bound with the outlier's column, bound without it) -- see deviation()."""
    fam = FAMILY[case]
    if np.dtype(dtype) == np.float64:
        return (1e-7, 1e-7) if fam in ("nb", "gp") else (1e-6, 1e-6)
    return FP32_BOUND[bound_class(case, nonneg, k)]


def bound_class(case, nonneg, k):
    return (FAMILY[case], "clamped" if nonneg else "free", "wide" if k > 64 else "k<=64")


_CACHE = {}


def problem(dtype, k, case):
    """(A, F, G, theta_row, theta_col) of a loss case in `dtype` (A.x holds values exactly representable in float32)."""
    key = ("P", np.dtype(dtype), k, case)
    if key not in _CACHE:
        lt, th, power, robust, kind = LOSS_CASES[case]
        A = edge_matrix(kind)
        if th == "col":
            A = A.transpose()
        F, G = factor(A.rows, k, dtype, *((RIDGE_DENSE, DENSE_F_SHIFT.get(k, 0)) if kind == "dense" else ()))
        rng = np.random.default_rng(7)
        theta = rng.uniform(2.0, 20.0, size=max(ROWS, COLS)).astype(dtype)
        _CACHE[key] = (A, F, G, theta[:A.rows] if th == "row" else None, theta[:A.cols] if th == "col" else None)
    return _CACHE[key]


def options(dtype, case, opt):
    """Keyword arguments of Context.solve_irls for a loss and an option case (scalars still doubles: the ABI casts them)."""
    lt, th, power, robust, kind = LOSS_CASES[case]
    return dict(BASE, **OPTION_CASES[opt], **LOSS_OVERRIDES.get(case, {}), loss_param=power, robust_delta=robust)


def reference(dtype, k, case, opt="base"):
    """(X, passes, stat, trace) of the float64 restatement, the scalar options as the kernel of `dtype` sees them."""
    key = ("R", np.dtype(dtype), k, case, opt)
    if key not in _CACHE:
        A, F, G, tr, tc = problem(dtype, k, case)
        kw = options(dtype, case, opt)
        trace = {}
        X, passes, stat = irls_half_update(
            A, F, G, loss_type=LOSS_CASES[case][0], dtype=dtype, l1=q(kw["l1"], dtype), l2=q(kw["l2"], dtype), nonneg=bool(kw["nonneg"]),
            cd_maxit=kw["cd_maxit"], irls_max_iter=kw["irls_max_iter"], irls_tol=q(kw["irls_tol"], dtype), theta_row=tr, theta_col=tc,
            power=q(kw["loss_param"], dtype), robust=q(kw["robust_delta"], dtype), trace=trace)
        trace.pop("Gw", None)                               # (n, k, k) per case: not kept
        _CACHE[key] = (X, passes, stat, trace)
    return _CACHE[key]


def all_cases(cd100=True):
    """Every (loss case, option case) of the matrix: each loss case with the base options, each option case on OPTION_LOSSES, the
    converging early-stop cases.  cd100 = False leaves out the 100-sweep case (it runs at CD100_KS only)."""
    out = [(c, "base") for c in MATRIX_LOSSES]
    out += [(c, o) for c in OPTION_LOSSES for o in OPTION_CASES if o not in ("base", "early2", "early3") and (cd100 or o != "cd100")]
    return out + [(c, o) for c, o in CONVERGING]


# the 100-sweep case: the smallest k of every kernel
CD100_KS = {np.dtype(np.float32): (4, 5, 33, 36, 65), np.dtype(np.float64): (2, 3, 33, 65)}


def cases_at(dtype, k):
    return all_cases(cd100=k in CD100_KS[np.dtype(dtype)])


def decisive_columns(dtype, k, case, opt):
    """Columns whose pass count cannot depend on rounding: cd_ref.decisive (the stop statistic outside irls_tol (1 +- EARLY_DELTA) at
    every pass the column ran) and, for fp32, every pass's decision unchanged by an absolute error e = EARLY_NOISE max|ref column| of
    both iterates: continue if  max_i (|dx_i| - 2 e) / (|x_old_i| + e + 1e-12) >= tol,  stop if
    max_i (|dx_i| + 2 e) / (max(|x_old_i| - e, 0) + 1e-12) < tol  (coordinates that are exactly 0 before and after the pass left out: a
    clamped coordinate stays clamped)."""
    from tests.cd_ref import decisive
    Xr, passes, stat, trace = reference(dtype, k, case, opt)
    tol = q(options(dtype, case, opt)["irls_tol"], dtype)
    dec = decisive(stat, tol, EARLY_DELTA[np.dtype(dtype)])
    e = EARLY_NOISE[np.dtype(dtype)] * np.abs(Xr).max(axis=1, keepdims=True)
    if EARLY_NOISE[np.dtype(dtype)] > 0:
        eps12 = float(np.dtype(dtype).type(1e-12))
        xo = np.zeros_like(Xr)
        for m, xn in enumerate(trace["X"]):
            ran = passes > m
            live = ~((xo == 0) & (xn == 0))
            dx = np.abs(xn - xo)
            lo = np.where(live, np.maximum(dx - 2 * e, 0) / (np.abs(xo) + e + eps12), 0.0).max(axis=1)
            hi = np.where(live, (dx + 2 * e) / (np.maximum(np.abs(xo) - e, 0) + eps12), 0.0).max(axis=1)
            dec &= ~ran | (lo >= tol) | (hi < tol)
            xo = xn
    return dec


def outlier_column(case):
    if LOSS_CASES[case][4] == "dense":
        return -1                                           # no outlier: both figures cover every column
    return OUTLIER[0] if LOSS_CASES[case][1] == "col" else OUTLIER[1]


def deviation(X, Xr, case, cols=None):
    """The two figures every bound of this file applies to: max|X - Xr| / max|Xr| over all columns, and the same over the columns
    other than the outlier's -- its iterate can be 1e3 times the others' and its passes swing between two states, so that one
    normalisation alone would hide every other column behind it.  cols (a mask): the deviation of these columns only, normalised
    as before."""
    E = np.abs(np.asarray(X, np.float64) - Xr)
    keep = np.arange(Xr.shape[0]) != outlier_column(case)
    if cols is not None:
        E = np.where(np.asarray(cols, bool)[:, None], E, 0.0)
    return E.max() / np.abs(Xr).max(), E[keep].max() / np.abs(Xr[keep]).max()


def within(dev, bnd):
    return dev[0] < bnd[0] and dev[1] < bnd[1]


LEFT_OUT = 3        # columns left out of an unclamped case: 4.5 % of 67


def kept_columns(dtype, k, case, opt):
    """The columns a case is compared on: all of them when clamped.  Without the clamp x changes sign and a reconstruction
    f . x can cancel: a rounding error of the dot product then grows by sum |f_i x_i| / |f . x| in mu and, the weights being
    ~ 1 / mu^p, by as much in the weight -- a single such entry moves its column by 1e-3 .. 1e-1 of max|ref| between two fp32
    evaluations (the fp32 oracle included), whatever the ridge and however short the CD solve.  The LEFT_OUT columns with the
    largest such factor over all passes and entries (irls_ref: trace["cancel"], float64 restatement alone) are left out."""
    trace = reference(dtype, k, case, opt)[3]
    n = len(trace["cancel"])
    if options(dtype, case, opt)["nonneg"]:
        return np.ones(n, bool)
    keep = np.ones(n, bool)
    keep[np.argsort(-trace["cancel"], kind="stable")[:LEFT_OUT]] = False
    return keep

