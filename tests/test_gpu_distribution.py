"""GPU checks of the distribution diagnostics (csrc/ops_distribution.hip) against the numpy restatement in tests/distribution_ref.py,
from the same fp64 model: sums and trimmed means to 1e-12 on real and synthetic data in sparse and dense form, exact medians on
integer data with dense ties, run-to-run bitwise identity, a sparse matrix with more than 2^31 entries, and the reference's R tests
of these functions restated with numpy-generated data of the same structure."""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import distribution_ref as R
from rcppml_amd import _abi
from rcppml_amd import distribution as D
from rcppml_amd import nmf as nmf_module
from rcppml_amd.data import CSC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


class Model:
    def __init__(self, w, d, h, loss_type=None):
        self.w, self.d, self.h = np.asarray(w, float), np.asarray(d, float), np.asarray(h, float)
        self.misc = {} if loss_type is None else {"loss_type": loss_type}


def golden(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return CSC(z["shape"], z["p"], z["i"], z["x"]).to_scipy()


def pbmc_slice():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = sp.csc_matrix((np.asarray(x, float), np.asarray(i), np.asarray(p)), shape=(m, n))
    return A[:300, :150].tocsc()


def rand_model(m, n, k, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return Model(g.uniform(0.05, 1, (m, k)) * scale, g.uniform(0.5, 2, k), g.uniform(0.05, 1, (k, n)) / k)


def synthetic(kind, m, n, seed):
    g = np.random.default_rng(seed)
    mu = g.uniform(0.1, 1, (m, 3)) @ g.uniform(0.1, 1, (3, n)) * 2
    if kind == "poisson":
        A = g.poisson(mu).astype(float)
    elif kind == "gamma":
        A = g.gamma(2.0, mu / 2.0)
    else:                                             # zero-inflated Poisson
        A = g.poisson(mu).astype(float) * (g.random((m, n)) > 0.3)
    return A


def rel(a, b, scale=None):
    a, b = np.asarray(a, float), np.asarray(b, float)
    s = np.abs(b) if scale is None else scale
    return float(np.max(np.abs(a - b) / np.maximum(s, 1e-300)))


def abi_model(model):
    return np.ascontiguousarray(model.w), np.ascontiguousarray(model.d), np.ascontiguousarray(model.h.T)


def check_all(A, model, powers=(0, 1, 2, 3, 1.5), tol=TOL):
    sparse = sp.issparse(A)
    m, n = A.shape
    W, d, H = abi_model(model)
    csc = CSC.from_scipy(A) if sparse else None
    dense = None if sparse else np.asarray(A, float)
    # score test: sums against math.fsum, relative to the sum of the absolute terms
    r = _abi.score_test_double(csc, dense, m, n, W.shape[1], W, d, H, list(powers))
    assert r["status"] == 0, r["error"]
    S, snb, N, integral = R.score_sums(A, model, powers)
    xo, mo = R.observed(A, model, 1e-6)
    assert r["count"] == N and r["all_integer"] == integral
    if N == 0:                                        # mean(numeric(0)) is NaN
        assert np.isnan(r["T"]).all() and np.isnan(r["T_nb"])
    for q, p in enumerate(powers if N else ()):
        scale = math.fsum(np.abs((xo - mo) ** 2 / R.rpow(mo, p) - 1.0)) / max(N, 1)
        assert abs(r["T"][q] - S[q] / max(N, 1)) <= tol * max(scale, 1e-300), (p, r["T"][q], S[q] / N)
    if N:
        scale = math.fsum(np.abs(((xo - mo) ** 2 - mo) / (mo * mo))) / N
        assert abs(r["T_nb"] - snb / N) <= tol * scale
    # zero inflation
    z = _abi.zero_inflation_double(csc, dense, m, n, W.shape[1], W, d, H)
    assert z["status"] == 0, z["error"]
    er, ec, orow, ocol = R.zero_counts(A, model)
    assert rel(z["expected_row"], er) <= tol and rel(z["expected_col"], ec) <= tol
    assert np.array_equal(z["observed_row"], orow) and np.array_equal(z["observed_col"], ocol)
    # dispersion, every variance power the R switch yields
    for p in (0, 1, 2, 3):
        ds = _abi.dispersion_double(csc, dense, m, n, W.shape[1], W, d, H, float(p))
        assert ds["status"] == 0, ds["error"]
        P = R.phi(A, model, p)
        assert rel(ds["row_phi"], [R.trimmed_mean(P[i]) for i in range(m)]) <= tol
        assert rel(ds["col_phi"], [R.trimmed_mean(P[:, j]) for j in range(n)]) <= tol
        assert rel(ds["global_phi"], R.trimmed_mean(P)) <= tol


@pytest.mark.parametrize("form", ["sparse", "dense"])
@pytest.mark.parametrize("name", ["hawaiibirds", "movielens", "pbmc3k"])
def test_real_data(name, form):
    A = pbmc_slice() if name == "pbmc3k" else golden(name)
    if name == "movielens":
        A = A[:, :600].tocsc()
    m, n = A.shape
    check_all(A if form == "sparse" else A.toarray(), rand_model(m, n, 8, 1, scale=float(A.data.mean())))


@pytest.mark.parametrize("kind", ["poisson", "gamma", "zip"])
@pytest.mark.parametrize("form", ["sparse", "dense"])
def test_synthetic(kind, form):
    A = synthetic(kind, 67, 131, 5)
    check_all(sp.csc_matrix(A) if form == "sparse" else A, rand_model(67, 131, 3, 2, scale=2.0))


@pytest.mark.parametrize("k", [1, 200])
def test_rank_extremes(k):
    A = synthetic("poisson", 70, 65, 9)
    check_all(sp.csc_matrix(A), rand_model(70, 65, k, 3, scale=2.0))
    check_all(A, rand_model(70, 65, k, 3, scale=2.0))


def test_edges_empty_rows_columns_and_nnz_zero():
    A = synthetic("poisson", 65, 129, 4)
    A[5, :] = 0
    A[:, 7] = 0
    A[:, 128] = 0
    check_all(sp.csc_matrix(A), rand_model(65, 129, 4, 5))
    check_all(sp.csc_matrix((1, 1)), rand_model(1, 1, 2, 6))
    check_all(sp.csc_matrix((33, 17)), rand_model(33, 17, 2, 6))
    check_all(np.zeros((3, 2)), rand_model(3, 2, 1, 6))


def test_integer_model_exact_medians():
    """Integer model on small integer data: mu and phi are exact, ties are dense; with trim just below 0.5 every trimmed mean is a
    single order statistic (the median of an odd count), which must be exactly the restatement's."""
    g = np.random.default_rng(11)
    m, n, k = 45, 101, 3
    model = Model(g.integers(0, 3, (m, k)), g.integers(1, 3, k), g.integers(0, 3, (k, n)))
    A = g.integers(0, 6, (m, n)).astype(float)
    W, d, H = abi_model(model)
    for form in ("sparse", "dense"):
        csc, dense = (CSC.from_scipy(sp.csc_matrix(A)), None) if form == "sparse" else (None, A)
        for p in (0, 1, 2):
            ds = _abi.dispersion_double(csc, dense, m, n, k, W, d, H, float(p), min_mu=0.5, trim=0.4999)
            assert ds["status"] == 0, ds["error"]
            P = R.phi(A, model, p, min_mu=0.5)
            assert np.array_equal(ds["row_phi"], np.median(P, axis=1))
            assert np.array_equal(ds["col_phi"], np.median(P, axis=0))
            assert ds["global_phi"] == np.median(P)
            # the default trim: p = 0 makes phi integral, so the trimmed means are exact too
            ds = _abi.dispersion_double(csc, dense, m, n, k, W, d, H, float(p), min_mu=0.5)
            if p == 0:
                assert np.array_equal(ds["row_phi"], [R.trimmed_mean(P[i]) for i in range(m)])
                assert np.array_equal(ds["col_phi"], [R.trimmed_mean(P[:, j]) for j in range(n)])
                assert ds["global_phi"] == R.trimmed_mean(P)


def test_runs_are_bitwise_identical():
    A = pbmc_slice()
    m, n = A.shape
    W, d, H = abi_model(rand_model(m, n, 10, 8, scale=float(A.data.mean())))
    csc = CSC.from_scipy(A)
    for dense in (None, A.toarray()):
        c = None if dense is not None else csc
        runs = [(_abi.score_test_double(c, dense, m, n, 10, W, d, H, [0, 1, 2, 3]),
                 _abi.zero_inflation_double(c, dense, m, n, 10, W, d, H),
                 _abi.dispersion_double(c, dense, m, n, 10, W, d, H, 1.0)) for _ in range(2)]
        (s1, z1, d1), (s2, z2, d2) = runs
        assert s1["T"].tobytes() == s2["T"].tobytes() and s1["T_nb"] == s2["T_nb"]
        for key in ("expected_row", "expected_col"):
            assert z1[key].tobytes() == z2[key].tobytes()
        for key in ("row_phi", "col_phi"):
            assert d1[key].tobytes() == d2[key].tobytes()
        assert d1["global_phi"] == d2["global_phi"]


def test_more_than_2_31_entries():
    m = n = 46341                                    # m * n = 2 147 488 281 > 2^31
    g = np.random.default_rng(3)
    per = 3
    rows = np.sort(np.stack([g.choice(m, per, replace=False) for _ in range(n)]), axis=1).ravel().astype(np.int32)
    p = np.arange(0, per * n + 1, per, dtype=np.int32)
    x = g.integers(1, 5, per * n).astype(float)
    csc = CSC((m, n), p, rows, x)
    model = rand_model(m, n, 2, 4, scale=0.5)
    W, d, H = abi_model(model)
    z = _abi.zero_inflation_double(csc, None, m, n, 2, W, d, H)
    assert z["status"] == 0, z["error"]
    ds = _abi.dispersion_double(csc, None, m, n, 2, W, d, H, 1.0)
    assert ds["status"] == 0, ds["error"]
    A = csc.to_scipy()
    Wd = model.w * model.d[None, :]
    for i in list(g.choice(m, 6, replace=False)) + [m - 1]:
        mu = Wd[i] @ model.h
        assert rel(z["expected_row"][i], np.exp(-np.maximum(mu, 1e-8)).sum()) <= TOL
        assert z["observed_row"][i] == n - A[i].nnz
        xrow = A[i].toarray().ravel()
        mu = np.maximum(mu, 1e-6)
        assert rel(ds["row_phi"][i], R.trimmed_mean((xrow - mu) ** 2 / mu)) <= TOL
    for j in list(g.choice(n, 6, replace=False)) + [n - 1]:
        mu = Wd @ model.h[:, j]
        assert rel(z["expected_col"][j], np.exp(-np.maximum(mu, 1e-8)).sum()) <= TOL
        assert z["observed_col"][j] == m - per
        xcol = A[:, j].toarray().ravel()
        mu = np.maximum(mu, 1e-6)
        assert rel(ds["col_phi"][j], R.trimmed_mean((xcol - mu) ** 2 / mu)) <= TOL


# ------------------------------------------------------------------ the public functions against the restatement
def test_public_functions_match_the_restatement():
    A = synthetic("zip", 80, 60, 12)
    model = rand_model(80, 60, 3, 13, scale=2.0)
    model.misc["loss_type"] = "gamma"
    for data in (A, sp.csc_matrix(A), CSC.from_scipy(sp.csc_matrix(A))):
        got, want = D.score_test_distribution(data, model, powers=(0, 1, 1.5, 2, 3)), R.score_test(data, model, (0, 1, 1.5, 2, 3))
        assert got["best_distribution"] == want["best_distribution"] and got["best_power"] == want["best_power"]
        assert [s["distribution"] for s in got["scores"]] == [s["distribution"] for s in want["scores"]]
        assert got["nb_diagnostic"]["overdispersed"] == want["nb_diagnostic"]["overdispersed"]
        got, want = D.diagnose_zero_inflation(data, model), R.zero_inflation(data, model)
        assert got["zi_mode"] == want["zi_mode"] and got["has_zi"] == want["has_zi"]
        assert abs(got["excess_zero_rate"] - want["excess_zero_rate"]) <= 1e-12
        got, want = D.diagnose_dispersion(data, model), R.dispersion(data, model)
        assert got["mode"] == want["mode"]
        assert rel(got["row_cv"], want["row_cv"]) <= 1e-10 and rel(got["col_cv"], want["col_cv"]) <= 1e-10


def test_na_condition_raises_like_r():
    A = np.abs(np.random.default_rng(1).normal(2, 1, (1, 30)))        # one row: sd(row_phi) is NA
    with pytest.raises(ValueError, match="missing value where TRUE/FALSE needed"):
        D.diagnose_dispersion(A, rand_model(1, 30, 1, 2))


# ------------------------------------------------------------------ restated reference tests (numpy data of the same structure)
def abs_rsparse(m, n, density, seed, scale=1.0):
    g = np.random.default_rng(seed)
    A = sp.random(m, n, density=density, random_state=g, format="csc", data_rvs=lambda s: np.abs(g.normal(size=s)))
    return (A * scale).tocsc()


def count_data(m, n, k, seed):
    g = np.random.default_rng(seed)
    return sp.csc_matrix(g.poisson(g.uniform(0, 2, (m, k)) @ g.uniform(0, 2, (k, n))).astype(float))


def gamma_data(m, n, k, seed):
    g = np.random.default_rng(seed)
    mu = g.uniform(0.5, 2, (m, k)) @ g.uniform(0.5, 2, (k, n))
    return g.gamma(2.0, mu / 2.0)


def check_auto(res, dists):
    assert set(res) == {"loss", "comparison", "models"}
    assert res["loss"] in dists
    rows = res["comparison"]
    assert len(rows) == len(dists) and len(res["models"]) == len(dists)
    assert all(set(r) == {"distribution", "nll", "df", "aic", "bic", "selected"} for r in rows)
    assert sum(r["selected"] for r in rows) == 1
    assert all(isinstance(mod, nmf_module.NMFModel) for mod in res["models"].values())
    assert all(np.isfinite([r["nll"], r["aic"], r["bic"]]).all() for r in rows)


def test_auto_distribution_file():
    """test_auto_distribution.R (whole file)."""
    A = abs_rsparse(50, 30, 0.3, 42, 10.0)
    res = D.auto_nmf_distribution(A, k=3, maxit=20)
    check_auto(res, ("mse", "gp", "nb"))
    best = [r for r in res["comparison"] if r["selected"]][0]
    assert best["bic"] == min(r["bic"] for r in res["comparison"])
    df = {r["distribution"]: r["df"] for r in res["comparison"]}
    assert df["gp"] > df["mse"] and df["nb"] > df["mse"]
    res = D.auto_nmf_distribution(A, k=3, distributions=("mse", "gp"), maxit=20)
    check_auto(res, ("mse", "gp"))
    res = D.auto_nmf_distribution(A, k=3, criterion="aic", maxit=20)
    best = [r for r in res["comparison"] if r["selected"]][0]
    assert best["aic"] == min(r["aic"] for r in res["comparison"])
    dense = np.abs(np.random.default_rng(42).normal(5, 1, (50, 30)))
    check_auto(D.auto_nmf_distribution(dense, k=3, maxit=20), ("mse", "gp", "nb"))
    res = D.auto_nmf_distribution(A, k=3, distributions="gp", maxit=20)
    assert len(res["comparison"]) == 1 and res["loss"] == "gp" and res["comparison"][0]["selected"]


def test_auto_distribution_verbose(capsys):
    D.auto_nmf_distribution(abs_rsparse(30, 20, 0.3, 42, 10.0), k=2, maxit=10, verbose=True)
    assert "Fitting NMF" in capsys.readouterr().out


def test_auto_models_equal_separate_fits():
    A = abs_rsparse(50, 30, 0.3, 7, 10.0)
    res = D.auto_nmf_distribution(A, k=3, maxit=20, seed=42, tol=1e-3)
    for dist, mod in res["models"].items():
        ref = nmf_module.nmf(A, 3, loss=dist, maxit=20, seed=42, verbose=False, tol=1e-3)
        assert np.array_equal(mod.w, ref.w) and np.array_equal(mod.h, ref.h) and np.array_equal(mod.d, ref.d)
        assert mod.misc["loss"] == ref.misc["loss"]


def test_distribution_api_score_test():
    """test_distribution_api.R :293-326."""
    A = count_data(40, 30, 2, 1)
    model = nmf_module.nmf(A, 2, maxit=15, tol=1e-4, seed=1, verbose=False)
    r = D.score_test_distribution(A, model)
    assert len(r["scores"]) >= 4 and r["best_distribution"] in ("gaussian", "gp", "gamma", "inverse_gaussian")
    G = gamma_data(30, 20, 2, 2)
    model = nmf_module.nmf(G, 2, maxit=10, tol=1e-4, seed=1, verbose=False)
    assert D.score_test_distribution(G, model)["best_distribution"] in ("gaussian", "gp", "gamma", "inverse_gaussian")
    A = count_data(30, 20, 2, 3)
    model = nmf_module.nmf(A, 2, maxit=10, tol=1e-4, seed=1, verbose=False)
    assert len(D.score_test_distribution(A, model, powers=(0, 1, 2))["scores"]) == 3


def test_distribution_api_auto_and_zero_inflation():
    """test_distribution_api.R :365-435; the nmf(zi = ...) fits are replaced by asserting a valid mode."""
    G = gamma_data(60, 40, 3, 4)
    res = D.auto_nmf_distribution(G, k=3, maxit=30, tol=1e-4, seed=42, verbose=False)
    assert isinstance(res["loss"], str)
    model = nmf_module.nmf(G, 3, loss=res["loss"], maxit=30, tol=1e-4, seed=42, verbose=False)
    assert model.w.shape[0] == 60
    A = abs_rsparse(50, 30, 0.3, 42)
    res = D.auto_nmf_distribution(A, k=3, maxit=20, tol=1e-3, seed=1, verbose=False)
    nmf_module.nmf(A, 3, loss=res["loss"], maxit=20, tol=1e-3, seed=1, verbose=False)
    g = np.random.default_rng(42)
    mu = g.uniform(size=(50, 3)) @ g.uniform(size=(3, 30))
    X = g.poisson(mu).astype(float)
    X[g.binomial(1, 0.3, X.shape) == 1] = 0
    A = sp.csc_matrix(X)
    model = nmf_module.nmf(A, 3, maxit=20, tol=1e-3, seed=1, verbose=False)
    assert D.diagnose_zero_inflation(A, model)["zi_mode"] in ("none", "row", "col")
    A = sp.csc_matrix(g.poisson(mu).astype(float))
    res = D.auto_nmf_distribution(A, k=3, maxit=20, tol=1e-3, seed=1, verbose=False)
    base = nmf_module.nmf(A, 3, loss=res["loss"], maxit=20, tol=1e-3, seed=1, verbose=False)
    assert D.diagnose_zero_inflation(A, base)["zi_mode"] in ("none", "row", "col")


def test_g1_g6_custom_powers():
    """test_g1_g6_fixes.R :89-114."""
    g = np.random.default_rng(99)
    A = np.maximum(g.gamma(0.5, 2.0, (60, 40)), 1e-8)
    res = D.auto_nmf_distribution(A, k=3, seed=42)
    nmf_module.nmf(A, 3, loss=res["loss"], maxit=20, tol=1e-3, seed=42, verbose=False)
    A = np.random.default_rng(42).gamma(2.0, 1.0, (40, 25))
    model = nmf_module.nmf(A, 2, maxit=10, tol=1e-3, seed=1, verbose=False)
    r = D.score_test_distribution(A, model, powers=(0.5, 1.5, 2.5))
    assert len(r["scores"]) == 3 and any(s["distribution"].startswith("power_") for s in r["scores"])


def test_coverage_gaps_dispersion():
    """test_coverage_gaps.R :91-120 (row_phi / col_phi are returned here, so their check is not vacuous)."""
    A = np.abs(np.random.default_rng(42).normal(2, 0.5, (60, 40)))
    model = nmf_module.nmf(A, 2, loss="mse", maxit=30, seed=1, verbose=False)
    r = D.diagnose_dispersion(A, model)
    assert r["mode"] in ("global", "per_row", "per_col")
    assert all(np.isfinite([r["global_phi"], r["row_cv"], r["col_cv"]]))
    assert np.isfinite(r["row_phi"]).all() and np.isfinite(r["col_phi"]).all()
    A = abs_rsparse(60, 40, 0.4, 42)
    model = nmf_module.nmf(A, 2, loss="gp", dispersion="per_row", maxit=20, seed=1, verbose=False)
    assert D.diagnose_dispersion(A.toarray(), model)["mode"] in ("global", "per_row", "per_col")
