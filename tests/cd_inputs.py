"""Shared inputs of tests/test_cd_ref_cpu.py, tests/test_gpu_cd_matrix.py and tests/test_gpu_masked_solve.py: problem builders,
option sets, seeds, the project's bounds and the float64 references of tests/cd_ref.py, computed once per process and shared.
numpy only: no torch, no GPU code, no oracle."""
import numpy as np

from tests.cd_ref import cd_solve_batch


def cd_problem(k, n, dtype, seed, ridge=0.0):
    """Gram and right-hand sides as in tests/test_gpu_kernels.py::_cd_problem, plus an optional ridge on the Gram (a fraction of its
    mean diagonal: 4k + 5 uniform samples give one dominant direction ~ k^2 / 4 against a bulk ~ k / 12, and long solves amplify fp32
    rounding by that ratio)."""
    rng = np.random.default_rng(seed)
    Fm = rng.uniform(size=(4 * k + 5, k))
    G = Fm.T @ Fm
    if ridge:
        G[np.diag_indices(k)] += ridge * np.mean(np.diag(G))
    G = G.astype(dtype)
    G[np.diag_indices(k)] += dtype(1e-15)
    B = (rng.standard_normal((n, k)) * 3 + 1).astype(dtype)
    # start values on the scale of the solution (its largest entry is about 8 / k here): a warm start two orders of magnitude off makes
    # b - G x0 cancel catastrophically, which measures fp32 rounding of the inputs rather than the kernel
    X0 = (rng.uniform(size=(n, k)) * min(1.0, 8.0 / k)).astype(dtype)
    return G, B, X0


def q(v, dtype):
    """A scalar option as the kernel of that dtype sees it (the C ABI takes doubles and casts them)."""
    return float(np.dtype(dtype).type(v))


def upper_bound_for(G, B):
    """An upper bound that binds on part of the entries: 0.4 x the largest entry of the unbounded cold 7-sweep solution (float64
    restatement), rounded to a float32 so that both dtypes see the same value."""
    X, _, _ = cd_solve_batch(G, B, None, zero_init=True, maxit=7)
    return float(np.float32(0.4 * X.max()))


def option_cases(dtype, ub):
    """The eleven option sets of test_options_every_instantiation: name -> keyword arguments of rcppml_hip_solve_cd (the
    restatement takes the same names).  Fixed 7 sweeps, no early exit."""
    l1p, l1, l2 = q(0.7, dtype), q(0.25 * ub, dtype), q(0.05, dtype)      # l1 inside the step on the scale of the solution
    base = dict(maxit=7, tol=0.0)
    return {
        "cold": dict(base, zero_init=1),
        "warm": dict(base, warm=1),
        "quirk": dict(base, warm=0, zero_init=0),
        "l1_pre": dict(base, warm=1, l1_pre=l1p),
        "l1_cd": dict(base, zero_init=1, l1_cd=l1),
        "l2_cd": dict(base, warm=1, l2_cd=l2),
        "l1_l2_ub": dict(base, warm=1, l1_cd=l1, l2_cd=l2, ub_cd=ub),
        "free": dict(base, zero_init=1, nonneg=0),
        "free_l2": dict(base, warm=1, nonneg=0, l2_cd=l2),
        "ub_cd": dict(base, zero_init=1, ub_cd=ub),
        "ub_post": dict(base, zero_init=1, ub_post=ub),
    }


def ref_kwargs(kw):
    """solve_cd keyword arguments -> cd_solve keyword arguments (ints -> bools)."""
    out = dict(kw)
    for name in ("warm", "zero_init", "nonneg"):
        if name in out:
            out[name] = bool(out[name])
    return out


def cd_tolerance(dtype, k, nonneg=True):
    """The project's existing bounds, relative to max|ref|: fp64 1e-9; fp32 3e-4, x 4 for 64 < k <= 128, x 16 for k > 128
    (test_fuzz_cd_auto); x 10 without non-negativity (test_cd_variants_options)."""
    if np.dtype(dtype) == np.float64:
        t = 1e-9
    else:
        t = 3e-4 * (16 if k > 128 else (4 if k > 64 else 1))
    return t * (1 if nonneg else 10)


# Shapes of the op-level CD matrix (tests/test_gpu_cd_matrix.py)
OPTION_KS = (1, 9, 16, 17, 32, 40, 48, 64, 70, 96, 100, 128, 129, 256)
OPTION_N = 129                      # a ragged tail for 16-, 32- and 64-column tiles
OPTION_RIDGE = 0.25                 # keeps the fp32 oracle within a quarter of the fp32 bound of the restatement (without: 0.27 at k = 48)
OPTION_NAMES = ("cold", "warm", "quirk", "l1_pre", "l1_cd", "l2_cd", "l1_l2_ub", "free", "free_l2", "ub_cd", "ub_post")
COUNT_KS = (48, 100)                # test_column_counts: nmax columns, seed 500 + k, OPTION_RIDGE; the first n of them are solved
COUNT_NS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
EARLY_KS = (9, 32, 64, 128)
EARLY_N = 129
# Ridge of the early-exit, work-order and AUTO-threshold inputs (solves of up to 100 sweeps).  Worst D (fp32 oracle against the float64
# restatement, as a fraction of the fp32 bound) over EARLY_KS x tol x cold / warm, with EARLY_SEED, by ridge:
#   0: 3.97   0.25: 6.92   0.5: 0.19   1.0: 0.06        (the worst class is k = 128, tol 1e-3, warm at every ridge)
# and without a ridge 7 % of the columns of k = 128 are non-decisive (limit 5 %).  Up to 0.25 the fp32 oracle itself leaves a
# non-decisive column one sweep away from the restatement; at tol = 1e-3 that one sweep moves the iterate by several bounds.  0.5
# meets the quarter, but at 0.19 of the bound; 1.0 is the next value tried.
EARLY_RIDGE = 1.0
# Seeds: 1000 + k unless the inputs miss a condition that tests/test_cd_ref_cpu.py asserts on the CPU.  One of them: on every decisive
# column the fp32 ORACLE reaches the float64 restatement's sweep count (else no fp32 kernel can be held to it); seed 1064 misses it.
EARLY_SEED = {9: 1009, 32: 1032, 64: 2064, 128: 1128}
EARLY_DELTA = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-2}
_CACHE = {}


def options_reference(dtype, k):
    """(G, B, X0, ub, cases, refs): inputs in `dtype`, refs[name] = (X, sweeps, stat) of the float64 restatement."""
    key = ("opt", np.dtype(dtype), k)
    if key not in _CACHE:
        G, B, X0 = cd_problem(k, OPTION_N, dtype, k, ridge=OPTION_RIDGE)
        ub = upper_bound_for(G, B)
        cases = option_cases(dtype, ub)
        refs = {name: cd_solve_batch(G, B, X0, **ref_kwargs(kw)) for name, kw in cases.items()}
        _CACHE[key] = (G, B, X0, ub, cases, refs)
    return _CACHE[key]


def early_reference(dtype, k, tol, warm):
    """(G, B, X0, kw, (X, sweeps, stat)) of an early-exit solve (maxit 100); tol as the kernel of that dtype sees it."""
    key = ("early", np.dtype(dtype), k, tol, warm)
    if key not in _CACHE:
        G, B, X0 = cd_problem(k, EARLY_N, dtype, EARLY_SEED[k], ridge=EARLY_RIDGE)
        kw = dict(warm=1 if warm else 0, zero_init=0 if warm else 1, maxit=100, tol=tol)
        rk = ref_kwargs(kw)
        rk["tol"] = q(tol, dtype)
        _CACHE[key] = (G, B, X0, kw, cd_solve_batch(G, B, X0, **rk))
    return _CACHE[key]


def count_reference(dtype, k):
    """(G, B, X0, X): the inputs of test_column_counts (COUNT_NS[-1] columns) and the float64 restatement of the warm 7-sweep
    solve.  Columns are independent: a run on the first n columns is compared with X[:n]."""
    key = ("count", np.dtype(dtype), k)
    if key not in _CACHE:
        G, B, X0 = cd_problem(k, COUNT_NS[-1], dtype, 500 + k, ridge=OPTION_RIDGE)
        _CACHE[key] = (G, B, X0, cd_solve_batch(G, B, X0, warm=True, maxit=7)[0])
    return _CACHE[key]


class Pattern:
    """Minimal CSC holder (p, i, x) for masked_half_update; the tests wrap the same arrays for the oracle."""
    def __init__(self, rows, cols, p, i, x):
        self.rows, self.cols = rows, cols
        self.p, self.i, self.x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)

    def transpose(self):
        cols_of = np.repeat(np.arange(self.cols, dtype=np.int32), np.diff(self.p))
        order = np.lexsort((cols_of, self.i))
        p = np.zeros(self.rows + 1, np.int32)
        np.add.at(p, self.i + 1, 1)
        return Pattern(self.cols, self.rows, np.cumsum(p), cols_of[order], self.x[order])


def masked_problem(k, seed, rows=90, cols=37):
    """A rows x cols sparse matrix and a mask of the same shape (rows sorted inside every column) with the edge columns the
    masked solve has to get right: column 0 is empty (mask not empty), column 1 has every stored entry masked, column 2 has masked
    rows that hold no stored entry (beside some that do), column 3 has an empty mask; the rest is random.  Returns (A, M, F, X0)
    in float64.  With 90 rows the Gram of F is singular from k = 90 on: the tests add a ridge to it (masked_gram)."""
    rng = np.random.default_rng(seed)
    ap, ai, ax, mp, mi = [0], [], [], [0], []
    for j in range(cols):
        cnt = 0 if j == 0 else int(rng.integers(3, 14))
        r = np.sort(rng.choice(rows, size=cnt, replace=False))
        if j == 0:
            m = np.sort(rng.choice(rows, size=3, replace=False))
        elif j == 1:
            m = r.copy()
        elif j == 2:
            free = np.setdiff1d(np.arange(rows), r)
            m = np.sort(np.concatenate([r[:2], rng.choice(free, size=3, replace=False)]))
        elif j == 3:
            m = np.zeros(0, np.int64)
        else:
            nm = int(rng.integers(0, 6))
            m = np.sort(rng.choice(rows, size=nm, replace=False))
        ai.append(r); ax.append(rng.uniform(0.1, 1.0, size=cnt)); ap.append(ap[-1] + cnt)
        mi.append(m); mp.append(mp[-1] + len(m))
    A = Pattern(rows, cols, ap, np.concatenate(ai), np.concatenate(ax))
    mi = np.concatenate(mi)
    M = Pattern(rows, cols, mp, mi, np.ones(len(mi)))
    F = rng.uniform(size=(rows, k))
    X0 = rng.uniform(size=(cols, k))
    return A, M, F, X0


def masked_gram(F, dtype, ridge=0.25):
    """G = F^T F + ridge * mean(diag) * I of the dtype-rounded F, rounded to dtype.  G_loc = G - sum_masked f f^T keeps the ridge
    whatever the mask takes away, so the Cholesky branch (and CD at k > rows) meets a well-conditioned matrix: without it fp32
    rounding is amplified by the condition number and no fixed bound holds (see test_target_regularisation in test_gpu_plugin.py)."""
    Fd = np.asarray(F, dtype).astype(np.float64)
    G = Fd.T @ Fd
    G[np.diag_indices(G.shape[0])] += ridge * np.mean(np.diag(G))
    return G.astype(dtype)
