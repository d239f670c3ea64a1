"""Zero-inflated GP / NB NMF without a device: the restatement (tests/zi_ref.py) against hand-worked cases, the pi initialisation, the
first ALS iteration against the oracle's plain IRLS fit, the new symbols, nmf_zi()'s validation and the refusals of the two entries
(every refusal happens before the device is touched, so these hold with and without one)."""
import os
import re

import numpy as np
import pytest

import zi_ref as Z
from oracle import oracle as O
from rcppml_amd import _abi
from rcppml_amd.zi import nmf_zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GP, NB, ROW, COL = Z.GP, Z.NB, Z.ROW, Z.COL


def _csc(dense, stored):
    """oracle Csc storing exactly the entries where `stored` is True (explicit zeros included)."""
    dense, stored = np.asarray(dense, np.float64), np.asarray(stored, bool)
    p, ii, xx = [0], [], []
    for j in range(dense.shape[1]):
        r = np.nonzero(stored[:, j])[0]
        ii += list(r)
        xx += list(dense[r, j])
        p.append(len(ii))
    return O.Csc(dense.shape, np.array(p, np.int32), np.array(ii, np.int32), np.array(xx, np.float64))


def _p0(s, dv, loss):
    if loss == NB:
        r = max(dv, 1e-10)
        return float(np.power(r / (r + s), r))
    return float(np.exp(-s / (1.0 + dv)))


def _z(p, p0):
    return p / (p + (1.0 - p) * p0 + 1e-300)


def _clamp(v):
    return min(max(v, 0.001), 0.999)


@pytest.mark.parametrize("loss", [GP, NB])
@pytest.mark.parametrize("mode", [ROW, COL])
def test_hand_worked_2x2(loss, mode):
    """2 x 2, k = 1, only (0, 0) stored.  a = W_T d = (3, 0.75), h = (1, 0.5): s(1,0) = 0.75, s(0,1) = 1.5, s(1,1) = 0.375."""
    A = _csc([[3.0, 0.0], [0.0, 0.0]], [[True, False], [False, False]])
    W_T, d, H = np.array([[2.0], [0.5]]), np.array([1.5]), np.array([[1.0], [0.5]])
    disp = np.array([0.25, 2.0])
    pi = np.array([0.2, 0.3])
    s10, s01, s11 = 0.75, 1.5, 0.375
    pr = (lambda i, j: pi[i]) if mode == ROW else (lambda i, j: pi[j])
    z10 = _z(pr(1, 0), _p0(s10, disp[1], loss))
    z01 = _z(pr(0, 1), _p0(s01, disp[0], loss))
    z11 = _z(pr(1, 1), _p0(s11, disp[1], loss))
    if mode == ROW:
        new = np.array([_clamp(z01 / 2.0), _clamp((z10 + z11) / 2.0)])
        q = lambda i, j: new[i]
    else:
        new = np.array([_clamp(z10 / 2.0), _clamp((z01 + z11) / 2.0)])
        q = lambda i, j: new[j]
    imp = np.array([[3.0, _z(q(0, 1), _p0(s01, disp[0], loss)) * s01],
                    [_z(q(1, 0), _p0(s10, disp[1], loss)) * s10, _z(q(1, 1), _p0(s11, disp[1], loss)) * s11]])
    got_pi, got_disp, got_imp = Z.zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters=1)
    assert np.abs(got_pi - new).max() <= 1e-15
    assert np.abs(got_imp - imp).max() <= 1e-15
    assert got_imp[0, 0] == 3.0 and np.array_equal(got_disp, disp)


@pytest.mark.parametrize("loss", [GP, NB])
@pytest.mark.parametrize("mode", [ROW, COL])
def test_hand_worked_3x2(loss, mode):
    """3 x 2, k = 2: column 0 fully stored (its pi_col is kept), row 2 holds an explicit stored zero at (2, 0); unstored: (0,1), (1,1), (2,1).
    a rows: (1, 0.5), (0.25, 1), (0.5, 0.5); h_1 = (0.5, 1): s(0,1) = 1*0.5 + 0.5*1 = 1, s(1,1) = 0.125 + 1 = 1.125, s(2,1) = 0.25 + 0.5 = 0.75."""
    A = _csc([[2.0, 0.0], [1.0, 0.0], [0.0, 0.0]], [[True, False], [True, False], [True, False]])
    W_T = np.array([[2.0, 0.25], [0.5, 0.5], [1.0, 0.25]])
    d = np.array([0.5, 2.0])
    H = np.array([[1.0, 1.0], [0.5, 1.0]])
    disp = np.array([0.5, 1.0, 4.0])
    pi = np.array([0.1, 0.2, 0.3]) if mode == ROW else np.array([0.25, 0.15])
    s = [1.0, 1.125, 0.75]
    p0 = [_p0(s[i], disp[i], loss) for i in range(3)]
    if mode == ROW:
        z = [_z(pi[i], p0[i]) for i in range(3)]
        new = np.array([_clamp(z[i] / 2.0) for i in range(3)])
        imp1 = [_z(new[i], p0[i]) * s[i] for i in range(3)]
    else:
        z = [_z(pi[1], p0[i]) for i in range(3)]
        new = np.array([pi[0], _clamp(((z[0] + z[1]) + z[2]) / 3.0)])          # column 0 has no unstored entry: kept
        imp1 = [_z(new[1], p0[i]) * s[i] for i in range(3)]
    imp = np.array([[2.0, imp1[0]], [1.0, imp1[1]], [0.0, imp1[2]]])
    got_pi, _, got_imp = Z.zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters=1)
    assert np.abs(got_pi - new).max() <= 1e-15
    assert np.abs(got_imp - imp).max() <= 1e-15
    assert np.array_equal(got_imp[:, 0], [2.0, 1.0, 0.0])
    # the per-entry functions agree with the column-at-a-time loops
    a = W_T * d[None, :]
    for i in range(3):
        assert abs(Z.s_entry(a[i], H[1]) - s[i]) <= 1e-15
        assert Z.p0_entry(s[i], disp[i], loss) == p0[i]
    # a second round and the GP theta floor
    p2, d2, _ = Z.zi_stage(A, W_T, d, H, disp, pi, loss, mode, em_iters=2, theta_min=0.75)
    assert np.array_equal(d2, np.maximum(disp, 0.75) if loss == GP else disp)
    assert p2.shape == new.shape and np.all((p2 >= 0.001) & (p2 <= 0.999))


def test_pi_init():
    """4 x 5: row 0 empty, row 1 full, (2, 0) an explicit stored zero (not a zero), column 4 empty."""
    dense = np.zeros((4, 5))
    stored = np.zeros((4, 5), bool)
    stored[1, :] = True
    dense[1, :] = [1, 2, 3, 4, 5]
    stored[2, 0] = True
    stored[3, 1] = stored[3, 2] = True
    dense[3, 1], dense[3, 2] = 7.0, 8.0
    stored[1, 4] = False
    dense[1, 4] = 0.0
    A = _csc(dense, stored)
    assert A.nnz == 7
    pr = Z.pi_init(A, ROW)
    assert np.array_equal(pr, [0.3, min(0.5 * (1 - 4 / 5), 0.3), min(0.5 * (1 - 1 / 5), 0.3), min(0.5 * (1 - 2 / 5), 0.3)])
    pc = Z.pi_init(A, COL)
    assert np.array_equal(pc, [0.25, 0.25, 0.25, min(0.5 * (1 - 1 / 4), 0.3), 0.3])
    full = _csc(np.ones((3, 2)), np.ones((3, 2), bool))
    assert np.array_equal(Z.pi_init(full, ROW), np.zeros(3)) and np.array_equal(Z.pi_init(full, COL), np.zeros(2))


@pytest.mark.parametrize("loss", [GP, NB])
def test_first_iteration_is_the_plain_fit(loss):
    A = Z.simulate_zi_data(30, 20, 2, dropout=0.2, seed=5)
    W0, H0 = O.init_factors(7, 2, 30, 20)
    ref = O.nmf_fit(A, W0, H0, max_iter=1, tol=0.0, loss_type=loss, dispersion_mode=2)
    for mode in (ROW, COL):
        r = Z.zi_fit(A, W0, H0, loss=loss, mode=mode, maxit=1)
        assert np.array_equal(r.W_T, ref.W_T) and np.array_equal(r.H, ref.H) and np.array_equal(r.d, ref.d)
        assert np.array_equal(r.theta, ref.theta) and r.loss == ref.loss
        assert not np.array_equal(r.pi, r.pi_init)


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name in ("rcppml_gpu_nmf_zi_double", "rcppml_gpu_zi_em_double"):
        assert re.search(r"RCPPML_GPU_API\s+void\s+%s\s*\(" % name, hdr)
        assert name in _abi.EXPORTED_SYMBOLS
        assert hasattr(_abi.lib(), name)
    import rcppml_amd
    assert "nmf_zi" in rcppml_amd.__doc__


def test_nmf_zi_validation_messages():
    X = Z.simulate_zi_data(12, 9, 2, seed=1).toarray()
    with pytest.raises(ValueError, match=re.escape("zi != 'none' requires loss='gp' or loss='nb'.")):
        nmf_zi(X, 2, loss="mse", zi="row")
    with pytest.raises(ValueError, match=re.escape("zi != 'none' requires loss='gp' or loss='nb'.")):
        nmf_zi(X, 2, loss="gamma", zi="col")
    with pytest.raises(ValueError, match=re.escape("'arg' should be one of 'none', 'row', 'col'")):
        nmf_zi(X, 2, zi="twoway")
    with pytest.raises(NotImplementedError, match="per_col"):
        nmf_zi(X, 2, zi="row", dispersion="per_col")
    with pytest.raises(NotImplementedError, match="fp64"):
        nmf_zi(X, 2, zi="row", precision="fp32")
    with pytest.raises(ValueError, match="zi_em_iters"):
        nmf_zi(X, 2, zi="row", zi_em_iters=0)


# ----------------------------------------------------------------------------- refusals at the ABI
M, N, K = 6, 5, 2


def _inputs():
    A = Z.simulate_zi_data(M, N, K, dropout=0.3, seed=3)
    W0, H0 = O.init_factors(11, K, M, N)
    return A, W0, H0


def _fit_refused(text, A=None, k=K, **kw):
    A0, W0, H0 = _inputs()
    A = A or A0
    W0, H0 = (W0, H0) if k == K else O.init_factors(11, k, M, N)
    W, H = W0.copy(), H0.copy()
    args = dict(zi_mode=1, zi_em_iters=1, loss_type=5, max_iter=2)
    args.update(kw)
    r = _abi.nmf_zi_double(A.p, A.i, A.x, M, N, k, W, H, **args)
    assert r["status"] == -1 and text in r["error"], r
    d, theta, pi, tl, pl, it, loss = r["buffers"]
    assert np.array_equal(W, W0) and np.array_equal(H, H0) and np.all(d == 1.0)
    assert np.all(theta == -7.0) and np.all(pi == -7.0) and (tl, pl, it, loss) == (-7, -7, -7, -7.0)


def _stage_refused(text, A=None, k=K, **kw):
    A0, W0, H0 = _inputs()
    A = A or A0
    W0, H0 = (W0, H0) if k == K else O.init_factors(11, k, M, N)
    args = dict(loss_type=5, zi_mode=1, zi_em_iters=1)
    args.update(kw)
    disp0 = np.full(M, 10.0)
    pi0 = np.full(M if args["zi_mode"] != 2 else N, 0.2)
    r = _abi.zi_em_double(A, M, N, k, W0, np.ones(k), H0, disp0, pi0, **args)
    assert r["status"] == -1 and text in r["error"], r
    pi, disp, imp = r["buffers"]
    assert np.array_equal(pi, pi0) and np.array_equal(disp, disp0) and np.all(imp == -7.0)


@pytest.mark.parametrize("refused", [_fit_refused, _stage_refused])
def test_abi_refusals(refused):
    refused("zi_mode=TWOWAY is disabled due to numerical instability on high-sparsity data. Use ZI_ROW or ZI_COL instead.", zi_mode=3)
    refused("zi_mode must be ROW (1) or COL (2)", zi_mode=0)
    refused("requires GP or NB loss", loss_type=0)
    refused("requires GP or NB loss", loss_type=6)
    refused("k must be in [1, 128]", k=129)
    refused("zi_em_iters must be >= 1", zi_em_iters=0)
    A, _, _ = _inputs()
    bad = O.Csc((M, N), A.p, A.i[::-1].copy(), A.x)                      # rows not increasing / out of order
    refused("malformed CSC", A=bad)
    p2 = A.p.copy()
    p2[1], p2[2] = p2[2] + 1, p2[1]
    bad2 = O.Csc.__new__(O.Csc)
    bad2.rows, bad2.cols, bad2.p, bad2.i, bad2.x = M, N, p2, A.i, A.x
    refused("malformed CSC", A=bad2)


def test_abi_refuses_per_col():
    _fit_refused("dispersion='per_col'", dispersion_mode=3)


def test_valid_call_without_device():
    """A valid call: BackendError from nmf_zi() and status -1 with nothing written when no device is present; on a device it runs."""
    A, W0, H0 = _inputs()
    if _abi.detect():
        mod = nmf_zi(A.toarray(), K, seed=1, maxit=2)
        assert "pi_row" in mod.misc and "pi_col" not in mod.misc
        return
    _fit_refused("no HIP device")
    _stage_refused("no HIP device")
    with pytest.raises(_abi.BackendError):
        nmf_zi(A.toarray(), K, seed=1, maxit=2)
