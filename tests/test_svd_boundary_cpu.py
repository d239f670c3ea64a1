"""CPU checks of the host boundary the fourteen SVD entries share (csrc/ops_svd.hip): the refusals every family raises, on the
sparse and the dense entry of each, leave every buffer untouched, and a call with two faults reports the one the boundary has
always reported.  The expected strings were recorded from the library before the boundary was written once; every check sits
before any device work, so no GPU is needed (and on a GPU machine no call gets as far as a launch)."""
import numpy as np
import pytest

from rcppml_amd import _abi

M, N = 6, 5
KB = 6                                      # buffers sized for the largest k_max a case hands over, min(m, n) + 1

K_RANGE = "k_max must be in [1, min(m, n)]"
COL_PTR = "col_ptr must start at 0 and end at nnz"
ROW_IDX = "row index out of range"
NULL_MATRIX = "null matrix"
RS_CONSTRAINTS = "the randomized method does not support element constraints (L1 / L2 / nonneg / upper bound)"

# family: (wrapper, the keywords of an accepted call, the output buffers it takes)
FAMILIES = {
    "pca": (_abi.svd_pca, dict(algorithm=0), ("U", "d", "V", "test_loss", "iters", "row_means")),
    "cv": (_abi.svd_cv, dict(test_fraction=0.1), ("U", "d", "V", "test_loss", "iters", "row_means")),
    "reg": (_abi.svd_reg, dict(L21=(0.1, 0.1)), ("U", "d", "V", "test_loss", "iters", "row_means")),
    "krylov": (_abi.svd_krylov, dict(nonneg=(True, True)), ("U", "d", "V", "dw", "row_means")),
    "randomized": (_abi.svd_randomized, dict(), ("U", "d", "V", "iters", "row_means")),
}
SIZES = dict(U=M * KB, d=KB, V=N * KB, test_loss=KB, iters=KB, dw=16, row_means=M)

# what every family refuses: (the faults of the call, the matrix forms it applies to, the message)
SHARED = [
    (dict(k=0), ("sparse", "dense"), K_RANGE),
    (dict(k=min(M, N) + 1), ("sparse", "dense"), K_RANGE),
    (dict(bad="col_ptr"), ("sparse",), COL_PTR),
    (dict(bad="row_idx"), ("sparse",), ROW_IDX),
    (dict(null=True), ("dense",), NULL_MATRIX),
    (dict(k=0, bad="col_ptr"), ("sparse",), K_RANGE),
    (dict(k=0, null=True), ("dense",), K_RANGE),
]
# two faults in one call, per family: which message wins
DOUBLE = {
    "pca": [
        (dict(k=6, test_fraction=0.1), ("sparse", "dense"), K_RANGE),
        (dict(k=6, algorithm=7), ("sparse", "dense"), K_RANGE),
        (dict(algorithm=7, test_fraction=0.1), ("sparse", "dense"), "algorithm must be 0 (deflation) .. 4 (krylov)"),
        (dict(test_fraction=0.1, bad="col_ptr"), ("sparse",),
         "test_fraction > 0 (cross-validation / auto-rank) is not supported on the GPU"),
        (dict(algorithm=2, nonneg=(True, False), null=True), ("dense",),
         "element constraints (L1 / L2 / nonneg / upper bound) need algorithm 0 (deflation) on the GPU"),
    ],
    "cv": [
        (dict(k=6, patience=0), ("sparse", "dense"), K_RANGE),
        (dict(patience=0, test_fraction=1.5), ("sparse", "dense"), "patience must be >= 1"),
        (dict(patience=0, bad="col_ptr"), ("sparse",), "patience must be >= 1"),
        (dict(test_fraction=1.5, null=True), ("dense",), "test_fraction must be in [0, 1)"),
        (dict(obs_mask=([0] * (N + 1), [], M + 1, N), bad="row_idx"), ("sparse",), "obs_mask dimensions must match the matrix"),
    ],
    "reg": [
        (dict(k=6, patience=0), ("sparse", "dense"), K_RANGE),
        (dict(patience=0, L21=(-1.0, 0.0)), ("sparse", "dense"), "patience must be >= 1"),
        (dict(patience=0, bad="col_ptr"), ("sparse",), "patience must be >= 1"),
        # the family's further terms are read after the matrix is attached and checked: the matrix's fault wins
        (dict(L21=(-1.0, 0.0), bad="col_ptr"), ("sparse",), COL_PTR),
        (dict(L21=(-1.0, 0.0), null=True), ("dense",), NULL_MATRIX),
        (dict(L21=(-1.0, 0.0), angular=(-1.0, 0.0)), ("sparse", "dense"), "L21 penalties must be non-negative and finite"),
    ],
    "krylov": [
        (dict(k=6, L1=(-1.0, 0.0)), ("sparse", "dense"), K_RANGE),
        (dict(L1=(-1.0, 0.0), upper_bound=(0.0, -1.0)), ("sparse", "dense"), "L1 penalties must be non-negative"),
        (dict(L1=(-1.0, 0.0), bad="col_ptr"), ("sparse",), "L1 penalties must be non-negative"),
        (dict(nonneg=(False, False), bad="row_idx"), ("sparse",),
         "the krylov method without element constraints is Lanczos: call rcppml_gpu_svd_pca_* with algorithm 2"),
        (dict(tol=-1.0, null=True), ("dense",), "tol must be non-negative"),
    ],
    "randomized": [
        (dict(k=6, nonneg=(True, False)), ("sparse", "dense"), K_RANGE),
        (dict(nonneg=(True, False), L21=(0.1, 0.0)), ("sparse", "dense"), RS_CONSTRAINTS),
        (dict(nonneg=(True, False), bad="col_ptr"), ("sparse",), RS_CONSTRAINTS),
        (dict(nan=True, bad="row_idx"), ("sparse",), ROW_IDX),                     # the finite check follows the CSC check
        (dict(nan=True, k=0), ("sparse", "dense"), K_RANGE),
        (dict(test_fraction=0.1, null=True), ("dense",),
         "the randomized method does not support test_fraction > 0 (cross-validation / auto-rank)"),
    ],
}
CASES = [(fam, form, dict(faults), msg) for fam in FAMILIES for faults, forms, msg in SHARED + DOUBLE[fam] for form in forms]


class NullMatrix:
    """The library with the first argument of every entry, the dense matrix, handed over as null: a raw call the wrappers
    cannot make themselves."""

    def __init__(self, real):
        self.real = real

    def __getattr__(self, name):
        f = getattr(self.real, name)
        return f if name == "rcppml_gpu_last_error" else lambda *a: f(None, *a[1:])


def refused(family, form, faults, precision):
    """One refused call on buffers pre-filled with 7: (result, buffers)."""
    call, kw, keys = FAMILIES[family]
    kw = dict(kw, **faults)
    k, bad, nan = kw.pop("k", 3), kw.pop("bad", None), kw.pop("nan", False)
    kw.pop("null", None)
    A = np.abs(np.random.default_rng(2).standard_normal((M, N))) + 0.5
    if nan:
        A[4, 2] = np.nan
    bufs = {key: np.full(SIZES[key], 7, np.int32 if key == "iters" else np.float64) for key in keys}
    if form == "dense":
        return call(A, k, dense=True, precision=precision, center=True, buffers=bufs, **kw), bufs
    p = np.arange(N + 1, dtype=np.int32) * M                   # every entry stored, column by column
    i = np.tile(np.arange(M, dtype=np.int32), N)
    if bad == "col_ptr":
        p[0] = 1
    if bad == "row_idx":
        i[3] = M
    return call((p, i, A.ravel(order="F"), M, N), k, precision=precision, center=True, buffers=bufs, **kw), bufs


@pytest.mark.parametrize("family, form, faults, msg", CASES, ids=lambda v: v if isinstance(v, str) and len(v) < 12 else None)
def test_refusal_and_untouched_buffers(family, form, faults, msg, monkeypatch):
    if faults.get("null"):
        monkeypatch.setattr(_abi, "lib", lambda real=_abi.lib(): NullMatrix(real))
    for precision in ("double", "float"):
        r, bufs = refused(family, form, faults, precision)
        assert (r["status"], r["error"]) == (-1, msg)
        assert all(np.all(b == 7) for b in bufs.values())
        assert (r["k"], r["frob"], r["wall_ms"]) == (0, 0.0, 0.0)
