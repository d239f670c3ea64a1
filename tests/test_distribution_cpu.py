"""CPU checks of the distribution diagnostics: the numpy restatement (tests/distribution_ref.py) against hand-worked answers, R's
trimmed-mean rule, labels, decision tables and NA errors, auto_nmf_distribution's arithmetic with a stubbed nmf(), what a stored
explicit zero counts as in each function, match.arg messages, the C declarations / exports and the refusals (decided before any
device work, nothing written).  No GPU needed."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import distribution_ref as R
from rcppml_amd import _abi
from rcppml_amd import distribution as D
from rcppml_amd import nmf as nmf_module
from rcppml_amd.data import CSC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcppml_gpu_score_test_double", "rcppml_gpu_zero_inflation_double", "rcppml_gpu_dispersion_double")


class Model:
    def __init__(self, w, d, h, loss_type=None, loss=None):
        self.w, self.d, self.h = np.asarray(w, float), np.asarray(d, float), np.asarray(h, float)
        self.misc = {}
        if loss_type is not None:
            self.misc["loss_type"] = loss_type
        if loss is not None:
            self.misc["loss"] = loss


# 4 x 3, rank 1: mu = 2 * w h^T = [[2,1,6],[4,2,12],[2,1,6],[2,1,6]]
X43 = np.array([[3, 0, 6], [4, 1, 10], [0, 0, 1], [2, 2, 0]], float)
M43 = Model([[1], [2], [1], [1]], [2], [[1, 0.5, 3]])


def test_hand_worked_score_test_dense():
    r = R.score_test(X43, M43, powers=(0, 1, 2))
    T = [s["T_stat"] for s in r["scores"]]
    assert T[0] == pytest.approx(62 / 12, rel=1e-14)
    assert T[1] == pytest.approx(4.5 / 12, rel=1e-14)
    assert T[2] == pytest.approx((5.5 + 13 / 18 - 12) / 12, rel=1e-14)
    assert r["best_power"] == 1 and r["best_distribution"] == "gp"
    assert r["nb_diagnostic"]["T_NB"] == pytest.approx(7 / 216, rel=1e-14)
    assert r["nb_diagnostic"]["overdispersed"] is False


def test_hand_worked_score_test_sparse():
    r = R.score_test(sp.csc_matrix(X43), M43, powers=(0,))
    assert r["scores"][0]["T_stat"] == pytest.approx((32 - 8) / 8, rel=1e-14)


def test_hand_worked_zero_inflation():
    er, ec, orow, ocol = R.zero_counts(X43, M43)
    e = np.exp(-np.array([[2, 1, 6], [4, 2, 12], [2, 1, 6], [2, 1, 6]], float))
    assert np.allclose(er, e.sum(1), rtol=1e-15) and np.allclose(ec, e.sum(0), rtol=1e-15)
    assert orow.tolist() == [1, 0, 2, 1] and ocol.tolist() == [1, 2, 1]
    assert R.zero_counts(sp.csc_matrix(X43), M43)[2].tolist() == [1, 0, 2, 1]


def test_hand_worked_dispersion():
    r = R.dispersion(X43, M43)                     # mse: phi = r^2 = [[1,1,0],[0,1,4],[4,1,25],[0,1,36]]
    assert np.allclose(r["row_phi"], [2 / 3, 5 / 3, 10, 37 / 3], rtol=1e-15)
    assert np.allclose(r["col_phi"], [5 / 4, 1, 65 / 4], rtol=1e-15)
    assert r["global_phi"] == pytest.approx(3.8, rel=1e-15)   # N = 12: order statistics 2..11


@pytest.mark.parametrize("N,lo,hi", [(1, 1, 1), (9, 1, 9), (10, 2, 9), (11, 2, 10), (19, 2, 18), (20, 3, 18)])
def test_trim_rule(N, lo, hi):
    assert R.trim_bounds(N, 0.1) == (lo, hi)
    x = np.random.default_rng(N).permutation(np.arange(1, N + 1)).astype(float)
    assert R.trimmed_mean(x) == pytest.approx((lo + hi) / 2, rel=1e-15)


def test_trim_rule_with_ties():
    x = np.array([3, 1, 100, 2, 1, 3, 2, 1, 3, 2], float)      # N = 10: ranks 2..9 of 1,1,1,2,2,2,3,3,3,100
    assert R.trimmed_mean(x) == pytest.approx(17 / 8, rel=1e-15)
    assert R.trimmed_mean(np.full(19, 7.25)) == 7.25
    x = np.array([0] * 5 + [9] * 15, float)                     # N = 20: ranks 3..18 -> three zeros, thirteen nines
    assert R.trimmed_mean(x) == pytest.approx(13 * 9 / 16, rel=1e-15)


def test_labels():
    for p, lab in ((0, "gaussian"), (1.0, "gp"), (2, "gamma"), (3, "inverse_gaussian"), (1.5, "power_1.5"), (0.5, "power_0.5"),
                   (2.5, "power_2.5"), (4, "power_4")):
        assert D.power_label(p) == lab == R.label(p)


def test_which_min_skips_nan():
    assert D.which_min([np.nan, 2.0, 1.0, 1.0]) == 2
    assert D.which_min([np.nan, np.nan]) is None


@pytest.mark.parametrize("rv", [0.0, 0.01, np.nan])
@pytest.mark.parametrize("cv", [0.0, 0.01, np.nan])
def test_zi_mode_table(rv, cv):
    def excess(v):
        if np.isnan(v):
            return np.array([0.3])
        return np.array([0.3 - np.sqrt(v / 2), 0.3 + np.sqrt(v / 2)])  # sample variance v
    rows, cols = excess(rv), excess(cv)
    try:
        want = R.zi_mode(True, rows, cols)
    except ValueError as e:
        with pytest.raises(ValueError, match=str(e)):
            D.zi_mode(True, rows, cols)
        assert np.isnan(cv) or (np.isnan(rv) and cv > 0.001)
        return
    assert D.zi_mode(True, rows, cols) == want
    assert want == ("col" if cv > 0.001 else "row")
    assert D.zi_mode(False, rows, cols) == "none"


@pytest.mark.parametrize("rcv", [0.2, 0.7, 0.9, np.nan])
@pytest.mark.parametrize("ccv", [0.2, 0.7, 0.9, np.nan])
def test_dispersion_mode_table(rcv, ccv):
    if np.isnan(rcv) or np.isnan(ccv):
        with pytest.raises(ValueError, match="missing value where TRUE/FALSE needed"):
            D.dispersion_mode(rcv, ccv, 0.5)
        return
    want = R.dispersion_mode(rcv, ccv, 0.5)
    assert D.dispersion_mode(rcv, ccv, 0.5) == want
    if rcv > 0.5 and ccv > 0.5:
        assert want == ("per_row" if rcv >= ccv else "per_col")
    elif rcv > 0.5 or ccv > 0.5:
        assert want == ("per_row" if rcv > 0.5 else "per_col")
    else:
        assert want == "global"


def test_loss_power_switch():
    for lt, p in (("mse", 0), ("gaussian", 0), ("gp", 1), ("kl", 1), ("gamma", 2), ("inverse_gaussian", 3), ("nb", 1),
                  ("tweedie", 0), (None, 0)):
        assert D.loss_power(Model([[1]], [1], [[1]], loss_type=lt)) == p


@pytest.fixture
def stub_nmf(monkeypatch):
    calls = []

    def fake(data, k, loss="mse", maxit=100, seed=None, verbose=False, **kw):
        calls.append(dict(loss=loss, k=k, maxit=maxit, seed=seed, verbose=verbose, kw=kw))
        loss_val = {"mse": 123.0, "gp": 456.0, "nb": 400.0}[loss]
        m, n = data.shape
        return Model(np.ones((m, k)), np.ones(k), np.ones((k, n)), loss_type=loss, loss=loss_val)

    monkeypatch.setattr(nmf_module, "nmf", fake)
    return calls


def test_auto_arithmetic(stub_nmf):
    A = sp.random(50, 30, density=0.3, random_state=1, format="csc") * 10
    res = D.auto_nmf_distribution(A, 3, maxit=20, seed=7, tol=1e-3)
    N = A.nnz
    rows = res["comparison"]
    assert [r["distribution"] for r in rows] == ["mse", "gp", "nb"]
    for r, loss in zip(rows, (123.0, 456.0, 400.0)):
        want = R.criteria(r["distribution"], loss, 3, 50, 30, N)
        for key in ("nll", "df", "aic", "bic"):
            assert r[key] == pytest.approx(want[key], rel=1e-15), key
    assert rows[0]["df"] == 3 * 80 + 1 and rows[1]["df"] == 3 * 80 + 50
    best = int(np.argmin([r["bic"] for r in rows]))
    assert res["loss"] == rows[best]["distribution"] and [r["selected"] for r in rows].count(True) == 1
    assert set(res["models"]) == {"mse", "gp", "nb"}
    assert all(c["maxit"] == 20 and c["seed"] == 7 and c["verbose"] is False and c["kw"] == {"tol": 1e-3} for c in stub_nmf)
    aic = D.auto_nmf_distribution(A, 3, criterion="aic")
    assert aic["loss"] == aic["comparison"][int(np.argmin([r["aic"] for r in aic["comparison"]]))]["distribution"]


def test_auto_dense_N_and_verbose(stub_nmf, capsys):
    A = np.abs(np.random.default_rng(0).normal(5, 1, (20, 10)))
    res = D.auto_nmf_distribution(A, 2, distributions="gp", verbose=True)
    out = capsys.readouterr().out
    assert "Fitting NMF with loss = gp ..." in out and "Best distribution: gp" in out and "( BIC )" in out
    assert res["comparison"][0]["bic"] == pytest.approx(2 * 456.0 + (2 * 30 + 20) * np.log(200.0), rel=1e-15)
    assert res["loss"] == "gp" and res["comparison"][0]["selected"]


def test_stored_explicit_zero_counts_differently(stub_nmf):
    # column 0 stores an explicit zero at row 1
    A = CSC((3, 2), [0, 2, 3], [0, 1, 2], [2.0, 0.0, 5.0])
    model = Model(np.ones((3, 1)), [1.0], np.ones((1, 2)))
    # which(data != 0): the stored zero is not observed by the score test
    x_obs, _ = R.observed(A, model, 1e-6)
    assert x_obs.tolist() == [2.0, 5.0]
    # diff(p) / tabulate(i): it is a nonzero for the zero counts
    _, _, orow, ocol = R.zero_counts(A, model)
    assert ocol.tolist() == [1, 2] and orow.tolist() == [1, 1, 1]
    # Matrix::nnzero: it is not a nonzero for N
    res = D.auto_nmf_distribution(A.to_scipy(), 1, distributions="gp")
    assert res["comparison"][0]["bic"] == pytest.approx(2 * 456.0 + (1 * 5 + 3) * np.log(2.0), rel=1e-15)


def test_match_arg_messages():
    A = np.ones((3, 3))
    with pytest.raises(ValueError, match="'arg' should be one of \"bic\", \"aic\""):
        D.auto_nmf_distribution(A, 1, criterion="x")
    with pytest.raises(ValueError, match="'arg' must be of length 1"):
        D.auto_nmf_distribution(A, 1, criterion=["bic", "x"])
    with pytest.raises(ValueError, match="'arg' should be one of \"mse\", \"gp\", \"nb\""):
        D.auto_nmf_distribution(A, 1, distributions=["zz"])
    with pytest.raises(ValueError, match="'arg' must be of length >= 1"):
        D.auto_nmf_distribution(A, 1, distributions=[])
    assert D.match_arg(("bic", "aic"), D.CRITERIA) == "bic"
    assert D.match_arg("a", D.CRITERIA) == "aic"
    assert D.match_arg(["g", "zz", "mse"], D.DISTRIBUTIONS, several_ok=True) == ["gp", "mse"]


def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name in NEW:
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[:5] == ["const int* col_ptr", "const int* row_idx", "const double* values", "int* nnz", "const double* dense"]
        assert args[-1] == "int* out_status"


def test_library_exports_the_entries():
    L = _abi.lib()
    for name in NEW:
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name), name


def _model43():
    return np.ascontiguousarray(M43.w), np.ascontiguousarray(M43.d), np.ascontiguousarray(M43.h.T)


def _calls(csc, dense, m=4, n=3, k=1, W=None, d=None, H=None, powers=(0, 1), trim=0.1):
    W0, d0, H0 = _model43()
    W = W0 if W is None else W
    d = d0 if d is None else d
    H = H0 if H is None else H
    return [_abi.score_test_double(csc, dense, m, n, k, W, d, H, powers),
            _abi.zero_inflation_double(csc, dense, m, n, k, W, d, H),
            _abi.dispersion_double(csc, dense, m, n, k, W, d, H, 0.0, trim=trim)]


def _untouched(r):
    for b in r["buffers"]:
        if isinstance(b, np.ndarray):
            assert np.all(b == -7.0)
        else:
            assert b == -7 or b == -7.0


def _refused(rs, pattern):
    for r in rs:
        assert r["status"] == -1 and re.search(pattern, r["error"]), r["error"]
        _untouched(r)


CSC43 = CSC.from_scipy(sp.csc_matrix(X43))


def test_refusals_write_nothing():
    _refused(_calls(CSC43, X43), "not both")
    _refused(_calls(None, None), "as a CSC or as a dense array")
    _refused(_calls(CSC43, None, m=0), "m, n and k")
    _refused(_calls(CSC43, None, k=0), "m, n and k")
    bad_rows = (CSC43.p, np.array([1, 0, 3, 0, 1, 3, 0, 1], np.int32)[:CSC43.nnz], CSC43.x)
    _refused(_calls(bad_rows, None), "strictly increasing|outside")
    _refused(_calls((CSC43.p, CSC43.i, np.where(CSC43.x == 6, np.nan, CSC43.x)), None), "non-finite")
    W = _model43()[0].copy()
    W[0, 0] = np.inf
    _refused(_calls(None, X43, W=W), "non-finite")
    r = _calls(None, X43, trim=0.5)[2]
    assert r["status"] == -1 and "trim" in r["error"]
    _untouched(r)
    W0, d0, H0 = _model43()
    r = _abi.score_test_double(None, X43, 4, 3, 1, W0, d0, H0, np.arange(9.0))
    assert r["status"] == -1 and "n_powers" in r["error"]
    _untouched(r)


def test_valid_call_without_device():
    """A valid call: refused with nothing written when no device is present; on a device it runs."""
    rs = _calls(CSC43, None) + _calls(None, X43)
    if _abi.detect():
        assert all(r["status"] == 0 for r in rs)
        return
    _refused(rs, "no HIP device")
    with pytest.raises(_abi.BackendError):
        D.score_test_distribution(X43, M43)
    with pytest.raises(_abi.BackendError):
        D.diagnose_zero_inflation(sp.csc_matrix(X43), M43)
    with pytest.raises(_abi.BackendError):
        D.diagnose_dispersion(X43, M43)
