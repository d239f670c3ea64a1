"""Zero-inflated GP / NB NMF on the device (rcppml_amd/csrc/ops_zi.hip) against the restatement of the reference's CPU fit
(tests/zi_ref.py): the E / M / impute stage entry by entry, whole fits, the first iteration against the plain fit, the properties the
reference's own tests ask for (tests/testthat/test_gpu_zi.R, test_zi_modes.R), repeatability and the memory guard.

Stage tolerance (the rule of DESIGN 4.11): device and restatement differ in summation order only, so the restatement is run twice per
input -- as written, and with columns, rows and factors visited in reverse and every accumulation in np.longdouble; delta is the largest
max|a - b| / max|b| over the outputs of the two, and the device gets 100 * max(delta, 2^-52).  delta never sees the device result.
Whole fits: the fp64 bars of DESIGN 7 (loss 1e-6 relative, factors 1e-6), the same 1e-6 for pi and for the dispersion vector (relative to
max(1, max|reference|): NB sizes run up to 1e6).  Their init seed (1, data seed 42) is one for which zi_fit agrees with itself across the
two summation orders to 3e-14 on every case, far inside a tenth of the bars: no column sits on the irls_tol stopping edge."""
import functools
import os

import numpy as np
import pytest

import zi_ref as Z
from oracle import oracle as O
from rcppml_amd import _abi
from rcppml_amd.data import CSC
from rcppml_amd.nmf import nmf
from rcppml_amd.zi import nmf_zi

pytestmark = pytest.mark.gpu
GP, NB, ROW, COL = Z.GP, Z.NB, Z.ROW, Z.COL
EPS = 2.0 ** -52


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-300))


# ----------------------------------------------------------------------------- 1. stage parity
def _stage_input(m, n, k, loss, mode, variant):
    """variant 0 (n > 1): column 0 fully stored (its pi_col is kept), the last column empty; variant 1 (m > 1): row 0 fully stored, the
    last row empty; otherwise a random pattern of density 0.3.
    Both: an explicit stored zero, pi at 0 / 0.001 / 0.999 / 1 (input and output meet both clamp bounds), GP theta below theta_min."""
    rng = np.random.default_rng(1000 * m + 10 * n + k + 7 * loss + 3 * mode + variant)
    stored = rng.random((m, n)) < 0.3
    if variant == 0 and n > 1:
        stored[:, 0] = True
        stored[:, n - 1] = False
    if variant == 1 and m > 1:
        stored[0, :] = True
        stored[m - 1, :] = False
    if m * n == 1:
        stored[0, 0] = variant == 0                                   # 1 x 1: the entry stored, then not
    dense = np.where(stored, rng.integers(1, 9, (m, n)).astype(np.float64), 0.0)
    si, sj = np.nonzero(stored)
    if len(si):
        dense[si[len(si) // 2], sj[len(si) // 2]] = 0.0               # an explicit stored zero
    p, ii, xx = [0], [], []
    for j in range(n):
        r = np.nonzero(stored[:, j])[0]
        ii += list(r)
        xx += list(dense[r, j])
        p.append(len(ii))
    A = O.Csc((m, n), np.array(p, np.int32), np.array(ii, np.int32), np.array(xx, np.float64))
    W_T, H, d = rng.random((m, k)), rng.random((n, k)), 0.5 + rng.random(k)
    disp = 0.5 + 19.5 * rng.random(m) if loss == NB else rng.random(m)
    L = m if mode == ROW else n
    pi = 0.3 * rng.random(L)
    for q, v in enumerate((0.0, 0.999, 0.001)):
        if q < L - 1:
            pi[q] = v
    pi[L - 1] = 1.0                                                   # variant 0 / COL and variant 1 / ROW: all unstored -> 0.999
    return A, stored, W_T, d, H, disp, pi


@pytest.mark.parametrize("em_iters", [1, 3])
@pytest.mark.parametrize("mode", [ROW, COL])
@pytest.mark.parametrize("loss", [GP, NB])
@pytest.mark.parametrize("k", [1, 3, 17, 33])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (65, 63), (130, 67)])
def test_stage_parity(shape, k, loss, mode, em_iters):
    m, n = shape
    theta_min = 0.3 if loss == GP else 0.0
    A, stored, W_T, d, H, disp, pi = _stage_input(m, n, k, loss, mode, 0 if em_iters == 1 else 1)
    ref = Z.zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters, theta_min)
    alt = Z.zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters, theta_min, acc=np.longdouble, reverse=True)
    delta = max(_rel(ref[0], alt[0]), _rel(ref[2], alt[2]))
    tol = 100.0 * max(delta, EPS)
    r = _abi.zi_em_double(A, m, n, k, W_T, d, H, disp, pi, loss, mode, em_iters, theta_min)
    assert r["status"] == 0, r["error"]
    dev = max(_rel(r["pi"], ref[0]), _rel(r["imputed"], ref[2]))
    print("zi stage %s k=%d loss=%d mode=%d em=%d: delta %.3e device %.3e (bound %.3e)" % (shape, k, loss, mode, em_iters, delta, dev, tol))
    assert dev <= tol
    assert np.array_equal(r["disp"], ref[1])
    dense = A.toarray()
    assert np.array_equal(r["imputed"][stored], dense[stored])          # bitwise A's values
    L = m if mode == ROW else n
    untouched = (stored.sum(axis=1) == n) if mode == ROW else (stored.sum(axis=0) == m)
    assert np.array_equal(r["pi"][untouched], pi[untouched])
    assert np.all((r["pi"][~untouched] >= 0.001) & (r["pi"][~untouched] <= 0.999)) and r["pi"].shape == (L,)


# ----------------------------------------------------------------------------- 2. whole fits
FIT_SHAPES = {"60x40": (60, 40, 3, 0.2), "50x35": (50, 35, 2, 0.15)}          # the shapes of the reference's test_gpu_zi.R
DATA_SEED, INIT_SEED = 42, 1


@functools.lru_cache(maxsize=None)
def _fit_data(name):
    m, n, k, dr = FIT_SHAPES[name]
    A = Z.simulate_zi_data(m, n, k, dropout=dr, seed=DATA_SEED)
    W0, H0 = O.init_factors(INIT_SEED, k, m, n)
    return A, W0, H0


@functools.lru_cache(maxsize=None)
def _fit_ref(name, loss, mode, maxit):
    A, W0, H0 = _fit_data(name)
    return Z.zi_fit(A, W0, H0, loss=loss, mode=mode, maxit=maxit, tol=0.0)


def _device_fit(name, loss, mode, maxit, **kw):
    A, W0, H0 = _fit_data(name)
    m, n, k, _ = FIT_SHAPES[name]
    W, H = W0.copy(), H0.copy()
    r = _abi.nmf_zi_double(A.p, A.i, A.x, m, n, k, W, H, zi_mode=mode, loss_type=loss, max_iter=maxit, tol=0.0, **kw)
    assert r["status"] == 0, r["error"]
    return r, W, H


@pytest.mark.parametrize("maxit", [2, 8])
@pytest.mark.parametrize("mode", [ROW, COL])
@pytest.mark.parametrize("loss", [NB, GP])
@pytest.mark.parametrize("name", sorted(FIT_SHAPES))
def test_whole_fit_parity(name, loss, mode, maxit):
    ref = _fit_ref(name, loss, mode, maxit)
    r, W, H = _device_fit(name, loss, mode, maxit)
    figs = dict(loss=abs(r["loss"] - ref.loss) / abs(ref.loss), W=np.abs(W - ref.W_T).max(), H=np.abs(H - ref.H).max(),
                d=np.abs(r["d"] - ref.d).max(), pi=np.abs(r["pi"] - ref.pi).max(),
                disp=np.abs(r["theta"] - ref.theta).max() / max(1.0, np.abs(ref.theta).max()))
    print("zi fit %s loss=%d mode=%d maxit=%d: %s" % (name, loss, mode, maxit, " ".join("%s %.2e" % kv for kv in figs.items())))
    assert r["iter"] == ref.iter == maxit
    assert all(v <= 1e-6 for v in figs.values()), figs
    assert np.abs(r["loss_history"] - ref.loss_history).max() / abs(ref.loss) <= 1e-6


# ----------------------------------------------------------------------------- 3. iteration 0 is the plain fit
def _as_product_csc(A):
    return CSC((A.rows, A.cols), A.p, A.i, A.x)


@pytest.mark.parametrize("zi", ["row", "col"])
@pytest.mark.parametrize("loss", ["nb", "gp"])
def test_first_iteration_is_the_plain_fit(loss, zi):
    A, _, _ = _fit_data("60x40")
    X = _as_product_csc(A)
    kw = dict(loss=loss, seed=3, maxit=1, tol=0.0, precision="fp64")
    plain = nmf(X, 3, **kw)
    mod = nmf_zi(X, 3, zi=zi, **kw)
    assert np.array_equal(mod.w, plain.w) and np.array_equal(mod.h, plain.h) and np.array_equal(mod.d, plain.d)
    pi = mod.misc["pi_" + zi]
    assert not np.array_equal(pi, Z.pi_init(A, ROW if zi == "row" else COL))


# ----------------------------------------------------------------------------- 4. properties
@pytest.mark.parametrize("zi", ["row", "col"])
@pytest.mark.parametrize("loss", ["nb", "gp"])
def test_properties(loss, zi):
    A, _, _ = _fit_data("60x40")
    X = _as_product_csc(A)
    m, n = X.shape
    mod = nmf_zi(X, 3, loss=loss, zi=zi, seed=42, maxit=10, tol=1e-4)
    assert np.all(np.isfinite(mod.w)) and np.all(mod.w >= 0) and np.all(np.isfinite(mod.h)) and np.all(mod.h >= 0)
    assert np.isfinite(mod.misc["loss"])
    assert ("pi_row" in mod.misc) != ("pi_col" in mod.misc)
    pi = mod.misc["pi_" + zi]
    stored = Z.stored_mask(A)
    has_zero = (stored.sum(axis=1) < n) if zi == "row" else (stored.sum(axis=0) < m)
    assert pi.shape == ((m,) if zi == "row" else (n,))
    assert np.all((pi[has_zero] >= 0.001) & (pi[has_zero] <= 0.999))
    plain = nmf(X, 3, loss=loss, seed=42, maxit=10, tol=1e-4, precision="fp64")
    assert mod.misc["loss"] != plain.misc["loss"]                              # 20 % dropout: the imputed half-updates move the fit


@pytest.mark.parametrize("zi", ["row", "col"])
def test_fully_stored_matrix(zi):
    rng = np.random.default_rng(9)
    D = rng.integers(1, 6, (20, 15)).astype(np.float64)
    D[3, 4] = 0.0                                                              # stored explicitly below: not a zero
    X = CSC((20, 15), np.arange(0, 301, 20, dtype=np.int32), np.tile(np.arange(20, dtype=np.int32), 15), D.T.reshape(-1))
    kw = dict(loss="nb", seed=5, maxit=1, tol=0.0, precision="fp64")
    mod, plain = nmf_zi(X, 2, zi=zi, **kw), nmf(X, 2, **kw)
    assert np.all(mod.misc["pi_" + zi] == 0.0)
    assert np.array_equal(mod.w, plain.w) and np.array_equal(mod.h, plain.h) and np.array_equal(mod.d, plain.d)


# ----------------------------------------------------------------------------- 5. repeatability
@pytest.mark.parametrize("mode", [ROW, COL])
def test_repeatable_and_grid_independent(mode, monkeypatch):
    m, n, k = 130, 67, 17
    A, stored, W_T, d, H, disp, pi = _stage_input(m, n, k, GP, mode, 0)
    monkeypatch.delenv("RCPPML_GPU_ZI_GRID", raising=False)
    runs = [_abi.zi_em_double(A, m, n, k, W_T, d, H, disp, pi, GP, mode, 2, 0.3) for _ in range(2)]
    for grid in ("1", "2", "5"):                                               # 6 tiles: one workgroup, a divisor, a non-divisor
        monkeypatch.setenv("RCPPML_GPU_ZI_GRID", grid)
        runs.append(_abi.zi_em_double(A, m, n, k, W_T, d, H, disp, pi, GP, mode, 2, 0.3))
    monkeypatch.delenv("RCPPML_GPU_ZI_GRID", raising=False)
    for r in runs:
        assert r["status"] == 0, r["error"]
        assert np.array_equal(r["pi"], runs[0]["pi"]) and np.array_equal(r["imputed"], runs[0]["imputed"])
        assert np.array_equal(r["disp"], runs[0]["disp"])
    a, Wa, Ha = _device_fit("50x35", NB, mode, 4)
    b, Wb, Hb = _device_fit("50x35", NB, mode, 4)
    monkeypatch.setenv("RCPPML_GPU_ZI_GRID", "1")
    c, Wc, Hc = _device_fit("50x35", NB, mode, 4)
    for r, W, H in ((b, Wb, Hb), (c, Wc, Hc)):
        assert np.array_equal(W, Wa) and np.array_equal(H, Ha) and np.array_equal(r["d"], a["d"])
        assert np.array_equal(r["pi"], a["pi"]) and np.array_equal(r["theta"], a["theta"]) and r["loss"] == a["loss"]


# ----------------------------------------------------------------------------- 6. the memory guard
def test_memory_guard():
    """200000 x 200000 with one stored entry: two fp64 m x n arrays alone are 640 GB.  Refused by arithmetic, buffers untouched."""
    m = n = 200000
    p = np.zeros(n + 1, np.int32)
    p[1:] = 1
    W0, H0 = np.full((m, 1), 0.5), np.full((n, 1), 0.5)
    W, H = W0.copy(), H0.copy()
    r = _abi.nmf_zi_double(p, np.zeros(1, np.int32), np.ones(1), m, n, 1, W, H, zi_mode=ROW, max_iter=2)
    assert r["status"] == -1 and "bytes of device memory" in r["error"], r
    need = int(r["error"].split("needs ")[1].split(" bytes")[0])
    assert need >= 2 * 8 * m * n + 2 * 4 * m * n + m * n // 8
    d, theta, pi, tl, pl, it, loss = r["buffers"]
    assert np.array_equal(W, W0) and np.array_equal(H, H0) and np.all(d == 1.0) and np.all(theta == -7.0) and np.all(pi == -7.0)
    assert (tl, pl, it, loss) == (-7, -7, -7, -7.0)
