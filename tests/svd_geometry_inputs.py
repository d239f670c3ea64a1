"""Shapes, inputs and case tables that take the SVD family's two-stage block reductions (rcppml_amd/csrc/kernels_svd.hip.h,
kernels_svd_reg.hip.h, kernels_svd_cv.hip.h) beyond one chunk of CH = WG * PER = 2048 elements: three and more blocks, a chunk that
is exactly full, a last chunk of one element, a different block count on either side, and the 256-row tiles of nmf_start_kernel.
Imported by tests/test_svd_geometry_cpu.py (the promises these inputs make, proved without a device) and
tests/test_gpu_svd_geometry.py (the device against the references).  No device code here.

The deflation references (plain, regularised, cross-validated) all come from svd_reg_ref.reg_deflation_svd: with its three terms
off it is svd_cv_ref.cv_deflation_svd and, without cross-validation, svd_ref.deflation_svd, operation for operation
(test_svd_reg_cpu.py and test_svd_cv_cpu.py hold them bitwise equal; test_svd_geometry_cpu.py does so again at one of these shapes),
and it is the one that also returns the per-iteration distances the fixed iteration counts are checked with.

Regenerate MEASURED with `PYTHONPATH=. python tests/svd_geometry_inputs.py`."""
import functools

import numpy as np

import svd_reg_ref as R
from svd_cv_ref import effective_cv_seed, holdout_grid, planted

CHUNK = 2048          # WG * PER of kernels_svd.hip.h; test_svd_geometry_cpu.py reads the header and fails if this stops being true
TILE = 256            # WG: the rows of one nmf_start_kernel block

# ------------------------------------------------------------------------------------------------ shapes
# name: m, n, planted singular values, noise, density of the CSC variant, rank compared, iterations, and why the shape is here.
# Spectra: the first k + 1 singular values of every matrix an entry factors from these (thinned, centred, held out, masked) have
# successive ratios <= 0.8 (test_svd_geometry_cpu.py asserts it).  Thinning at density p scales the planted values by p and adds a
# bulk of about sqrt(p (1 - p)) |sig| (1 / sqrt(m) + 1 / sqrt(n)); on the two 63-wide shapes that bulk swallows a fourth value at any
# density worth calling sparse, so they compare k = 2; the two wide shapes hold four values clear of it and compare k = 3.
# Iterations: fixed, tol = 0.  No iteration may come within 100 eps (float32: 1.2e-5) of convergence, or a rounded-negative distance
# could end a factor in one precision and not in the other; with ratios of 0.75 the distance 1 - |u . u_old| falls by three to ten
# times an iteration and passes 1.2e-5 in the fifth or sixth, so the count is four (the smallest distance of any case is then
# 7.8e-5; ITERS below takes one more off the case that came closer).  The issue's "about 10" would need ratios above 0.8.  The degenerate shapes converge in their first iteration by construction (a one-element factor is +-1), so they run one
# iteration: at max_iter = 1 a converged iteration and an unconverged one both count one.
SHAPES = {
    "2048x2049": dict(m=2048, n=2049, sig=(400.0, 300, 225, 168), noise=0.05, density=0.4, k=3, iters=4,
                      why="a full chunk with no tail on m; a second block of one element on n"),
    "4097x63": dict(m=4097, n=63, sig=(400.0, 280, 190), noise=0.05, density=0.6, k=2, iters=4,
                    why="three blocks on m, the last of one element; n below one wavefront (defl_u_kernel's grid-stride v)"),
    "63x6145": dict(m=63, n=6145, sig=(400.0, 280, 190), noise=0.05, density=0.6, k=2, iters=4,
                    why="four blocks on n, the last of one element; m below one wavefront"),
    "2051x4099": dict(m=2051, n=4099, sig=(400.0, 300, 225, 168), noise=0.05, density=0.4, k=3, iters=4,
                      why="two blocks on m and three on n: a kernel that mixes the two counts is wrong here"),
}
# the degenerate side: plain deflation and Lanczos only, centre off, k = 1
DEGENERATE = {
    "1x2049": dict(m=1, n=2049, sig=(400.0,), noise=0.05, density=0.5, k=1, iters=1, why="one row, two blocks on n"),
    "2049x1": dict(m=2049, n=1, sig=(400.0,), noise=0.05, density=0.5, k=1, iters=1, why="one column, two blocks on m"),
}
# A centred case factors planted() plus the constant LEVEL / sqrt(m n), a rank-one term that centring removes again.  Without it the
# row means of a planted matrix are sums that cancel (|mean| a hundredth of the entries and less), and the project's rtol = 1e-12
# on row_means would measure the order in which a row is added -- storage order on the host, pairwise in numpy -- instead of the
# value.  With it a row's mean is at least a third of its mean magnitude.  An uncentred case factors planted() as it is.
LEVEL = 520.0
ALL_SHAPES = dict(SHAPES, **DEGENERATE)
KINDS = ("csc", "dense")
EMPTY_ROW, EMPTY_COL = 7, 3                     # of the 2051 x 4099 pattern
NMF_SHAPES = {"513x257": (513, 257), "257x513": (257, 513)}      # len 513: three row blocks, one row in the last; 257: two
NMF_RANKS = (5, 33)


def nblk(length, chunk=CHUNK):
    return -(-length // chunk)


@functools.lru_cache(maxsize=None)
def shape_input(shape, kind, level=False):
    """(A with unstored entries 0, stored pattern or None for the dense entries).  planted() as it is for dense (level: on LEVEL, for
    the centred cases); thinned with a seeded Bernoulli pattern for csc, as svd_reg_ref.shape_input does."""
    s = ALL_SHAPES[shape]
    A = planted(s["m"], s["n"], s["sig"], 3 + s["m"], noise=s["noise"])
    if level:
        A = A + LEVEL / np.sqrt(s["m"] * s["n"])
    if kind == "dense":
        return A, None
    keep = np.random.default_rng(7 + s["n"]).random(A.shape) < s["density"]
    if shape == "2051x4099":
        keep[EMPTY_ROW, :] = False
        keep[:, EMPTY_COL] = False
    if shape in DEGENERATE:
        keep[0, 0] = keep[-1, -1] = True         # the one-element chunk holds a stored entry
    A = A * keep
    A.setflags(write=False)
    keep.setflags(write=False)
    return A, keep


# ------------------------------------------------------------------------------------------------ deflation family
CONSTRAINTS = {"free": dict(), "l1nn": dict(L1=(0.02, 0.02), nonneg=(True, True))}
SEED = 5

# plain deflation (_abi.svd_pca, algorithm 0): ("defl", shape, kind, center, constraints)
DEFLATION_CASES = ([("defl", s, kd, c, cons) for s in SHAPES for kd in KINDS for c in (False, True) for cons in CONSTRAINTS] +
                   [("defl", s, kd, False, cons) for s in DEGENERATE for kd in KINDS for cons in CONSTRAINTS])
# regularised deflation (_abi.svd_reg): every term on at once, svd_reg_ref's two "all" parameter sets: ("reg", shape, kind, params)
REG_CASES = [("reg", s, kd, p) for s in ("2051x4099", "4097x63") for kd in KINDS for p in ("all_l1_cv", "all_mask")]
# cross-validated deflation (_abi.svd_cv): ("cv", shape, variant)
CV_VARIANTS = {
    "csc": dict(kind="csc", mask_zeros=False),
    "csc_mask_zeros": dict(kind="csc", mask_zeros=True),
    "dense": dict(kind="dense", mask_zeros=False),
    "csc_obs_mask_center": dict(kind="csc", mask_zeros=False, mask=True, center=True),
}
CV_CASES = [("cv", s, v) for s in ("2051x4099", "63x6145") for v in CV_VARIANTS]
CV_KW = dict(test_fraction=0.1, patience=3)
MASK_DENSITY = 0.05
PARITY_CASES = DEFLATION_CASES + REG_CASES + CV_CASES
# Lanczos (_abi.svd_pca, algorithm 2) against numpy's dense SVD: (shape, kind, center)
LANCZOS_CASES = ([(s, kd, c) for s in SHAPES for kd in KINDS for c in (False, True)] +
                 [(s, kd, False) for s in DEGENERATE for kd in KINDS])
# NMF start (_abi.nmf_svd_init): (matrix, rank, kind)
NMF_CASES = [(key, k, kd) for key in NMF_SHAPES for k in NMF_RANKS for kd in KINDS]
# one CSC case per entry at 2051 x 4099 for the two-runs-are-bitwise-equal test
DETERMINISM_CASES = [("defl", "2051x4099", "csc", True, "l1nn"), ("reg", "2051x4099", "csc", "all_l1_cv"),
                     ("cv", "2051x4099", "csc_obs_mask_center")]
# fewer iterations where a factor of the restatement comes within 100 eps (float32) of convergence before the shape's count
ITERS = {("defl", "4097x63", "dense", False, "l1nn"): 3}        # 2.5e-5 in its fourth iteration


def case_id(case):
    return "-".join("center" if p is True else "raw" if p is False else str(p) for p in case)


def lanczos_k(shape):
    s = ALL_SHAPES[shape]
    return 5 if min(s["m"], s["n"]) >= 5 else 1


def case_shape(case):
    return case[1]


def case_kind(case):
    return CV_VARIANTS[case[2]]["kind"] if case[0] == "cv" else case[2]


def case_k(case):
    return ALL_SHAPES[case[1]]["k"]


def case_center(case):
    return bool(case[3]) if case[0] == "defl" else bool(CV_VARIANTS[case[2]].get("center")) if case[0] == "cv" else False


def case_iters(case):
    return ITERS.get(case, ALL_SHAPES[case[1]]["iters"])


@functools.lru_cache(maxsize=None)
def geometry_graphs(m, n):
    """svd_reg_ref.shape_graphs' construction at these dimensions: ring Laplacians with lambda * lambda_max_bound = GRAPH_BUDGET."""
    gu, gv = R.ring_laplacian(m, 21), R.ring_laplacian(n, 22)
    return gu, gv, R.GRAPH_BUDGET / R.lambda_max_bound(gu), R.GRAPH_BUDGET / R.lambda_max_bound(gv)


@functools.lru_cache(maxsize=None)
def obs_mask(m, n):
    mask = np.random.default_rng(31).random((m, n)) < MASK_DENSITY
    mask.setflags(write=False)
    return mask


def case_kwargs(case):
    """(A, stored, keywords of reg_deflation_svd) of one parity case: tol = 0, case_iters() iterations."""
    A, keep = shape_input(case_shape(case), case_kind(case), case_center(case))
    kw = dict(tol=0.0, maxit=case_iters(case), seed=SEED)
    if case[0] == "defl":
        kw.update(center=case[3], **CONSTRAINTS[case[4]])
    elif case[0] == "reg":
        p = dict(R.PARAMS[case[3]])
        assert p.pop("graphs") == "uv" and not p.get("center")
        gu, gv, lu, lv = geometry_graphs(*A.shape)
        kw.update(graph_u=gu, graph_v=gv, graph_lambda=(lu, lv))
        if p.pop("mask", False):
            kw["obs_mask"] = obs_mask(*A.shape)
        kw.update(p)
    else:
        v = dict(CV_VARIANTS[case[2]])
        v.pop("kind")
        if v.pop("mask", False):
            kw["obs_mask"] = obs_mask(*A.shape)
        kw.update(CV_KW, **v)
    return A, keep, kw


@functools.lru_cache(maxsize=None)
def case_ref(case, dtype=np.float64):
    A, keep, kw = case_kwargs(case)
    return R.reg_deflation_svd(A, case_k(case), stored=keep, dtype=dtype, **kw)


def factored_matrix(case):
    """The matrix the entry's products run on: obs-masked and held-out entries zeroed, row means subtracted when centred."""
    A, keep, kw = case_kwargs(case)
    m, n = A.shape
    pattern = np.ones((m, n), bool) if keep is None else keep
    At = A.copy()
    if kw.get("obs_mask") is not None:
        At[kw["obs_mask"] & pattern] = 0
    if kw.get("test_fraction", 0) > 0:
        At[holdout_grid(m, n, effective_cv_seed(kw["seed"], kw.get("cv_seed", 0)), kw["test_fraction"]) & pattern] = 0
    if kw.get("center"):
        At = At - A.mean(axis=1, keepdims=True)
    return At


@functools.lru_cache(maxsize=None)
def lanczos_ref(shape, kind, center):
    """(the matrix Lanczos factors, its singular values by numpy, the row means)."""
    A, _ = shape_input(shape, kind, center)
    D = A - A.mean(axis=1, keepdims=True) if center else A
    return D, np.linalg.svd(D, compute_uv=False), A.mean(axis=1)


# The restatement's own float32-vs-float64 deviation on each parity case (svd_reg_ref.deviation: u, d and v, each relative to its
# largest reference magnitude), at case_iters() iterations and tol = 0: reg_deflation_svd(dtype = np.float32) against
# reg_deflation_svd(dtype = np.float64), rounded up to three digits.  The fp32 device is held to four times these
# (tests/test_gpu_svd_geometry.py).  Regenerate with `PYTHONPATH=. python tests/svd_geometry_inputs.py`.
MEASURED = {
    ('defl', '2048x2049', 'csc', False, 'free'): 3.56e-07,
    ('defl', '2048x2049', 'csc', False, 'l1nn'): 3.69e-07,
    ('defl', '2048x2049', 'csc', True, 'free'): 5.62e-07,
    ('defl', '2048x2049', 'csc', True, 'l1nn'): 5.11e-07,
    ('defl', '2048x2049', 'dense', False, 'free'): 5.41e-07,
    ('defl', '2048x2049', 'dense', False, 'l1nn'): 5.50e-07,
    ('defl', '2048x2049', 'dense', True, 'free'): 6.33e-07,
    ('defl', '2048x2049', 'dense', True, 'l1nn'): 9.28e-07,
    ('defl', '4097x63', 'csc', False, 'free'): 5.54e-07,
    ('defl', '4097x63', 'csc', False, 'l1nn'): 5.55e-07,
    ('defl', '4097x63', 'csc', True, 'free'): 9.35e-07,
    ('defl', '4097x63', 'csc', True, 'l1nn'): 8.07e-06,
    ('defl', '4097x63', 'dense', False, 'free'): 5.50e-07,
    ('defl', '4097x63', 'dense', False, 'l1nn'): 3.43e-07,
    ('defl', '4097x63', 'dense', True, 'free'): 8.06e-07,
    ('defl', '4097x63', 'dense', True, 'l1nn'): 5.45e-06,
    ('defl', '63x6145', 'csc', False, 'free'): 1.61e-07,
    ('defl', '63x6145', 'csc', False, 'l1nn'): 1.52e-07,
    ('defl', '63x6145', 'csc', True, 'free'): 1.51e-07,
    ('defl', '63x6145', 'csc', True, 'l1nn'): 2.30e-07,
    ('defl', '63x6145', 'dense', False, 'free'): 1.74e-07,
    ('defl', '63x6145', 'dense', False, 'l1nn'): 2.84e-07,
    ('defl', '63x6145', 'dense', True, 'free'): 1.85e-07,
    ('defl', '63x6145', 'dense', True, 'l1nn'): 2.44e-07,
    ('defl', '2051x4099', 'csc', False, 'free'): 8.24e-07,
    ('defl', '2051x4099', 'csc', False, 'l1nn'): 3.97e-07,
    ('defl', '2051x4099', 'csc', True, 'free'): 5.69e-07,
    ('defl', '2051x4099', 'csc', True, 'l1nn'): 9.89e-07,
    ('defl', '2051x4099', 'dense', False, 'free'): 4.23e-07,
    ('defl', '2051x4099', 'dense', False, 'l1nn'): 1.56e-06,
    ('defl', '2051x4099', 'dense', True, 'free'): 4.11e-06,
    ('defl', '2051x4099', 'dense', True, 'l1nn'): 3.52e-05,
    ('defl', '1x2049', 'csc', False, 'free'): 8.68e-08,
    ('defl', '1x2049', 'csc', False, 'l1nn'): 9.01e-08,
    ('defl', '1x2049', 'dense', False, 'free'): 7.10e-08,
    ('defl', '1x2049', 'dense', False, 'l1nn'): 6.82e-08,
    ('defl', '2049x1', 'csc', False, 'free'): 9.21e-08,
    ('defl', '2049x1', 'csc', False, 'l1nn'): 4.24e-08,
    ('defl', '2049x1', 'dense', False, 'free'): 6.83e-08,
    ('defl', '2049x1', 'dense', False, 'l1nn'): 1.04e-07,
    ('reg', '2051x4099', 'csc', 'all_l1_cv'): 6.10e-07,
    ('reg', '2051x4099', 'csc', 'all_mask'): 4.14e-07,
    ('reg', '2051x4099', 'dense', 'all_l1_cv'): 4.34e-07,
    ('reg', '2051x4099', 'dense', 'all_mask'): 4.89e-07,
    ('reg', '4097x63', 'csc', 'all_l1_cv'): 3.99e-07,
    ('reg', '4097x63', 'csc', 'all_mask'): 4.35e-07,
    ('reg', '4097x63', 'dense', 'all_l1_cv'): 5.14e-07,
    ('reg', '4097x63', 'dense', 'all_mask'): 4.26e-07,
    ('cv', '2051x4099', 'csc'): 5.10e-07,
    ('cv', '2051x4099', 'csc_mask_zeros'): 5.12e-07,
    ('cv', '2051x4099', 'dense'): 5.12e-07,
    ('cv', '2051x4099', 'csc_obs_mask_center'): 2.25e-06,
    ('cv', '63x6145', 'csc'): 1.74e-07,
    ('cv', '63x6145', 'csc_mask_zeros'): 1.80e-07,
    ('cv', '63x6145', 'dense'): 2.37e-07,
    ('cv', '63x6145', 'csc_obs_mask_center'): 1.64e-07,
}


def measured(case):
    return R.deviation(case_ref(case, np.float32), case_ref(case, np.float64))


if __name__ == "__main__":
    print("MEASURED = {")
    for c in PARITY_CASES:
        dev = measured(c)
        e = int(np.floor(np.log10(dev)))
        print("    %r: %.2fe%03d," % (c, np.ceil(dev / 10.0 ** e * 100) / 100, e))     # rounded up
        case_ref.cache_clear()
    print("}")
