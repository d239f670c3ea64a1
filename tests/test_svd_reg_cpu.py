"""CPU checks of the L21 / angular / graph-regularised deflation SVD: the numpy restatement (tests/svd_reg_ref.py, the GPU path's
parity target) against svd_cv_ref and against brute-force element loops, the conditions its parity and convergence cases must
meet, R's validation messages and routing for the new arguments, and the entries' refusals that hold before any device work.
No GPU needed."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import svd_cv_ref as C
import svd_reg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("cv", [False, True])
def test_with_every_term_off_the_restatement_is_svd_cv_ref(name, cv):
    A, keep = (C.dense_input(), None) if name == "dense" else C.sparse_input()
    kw = dict(C.CV_KW) if cv else {}
    k = C.K_MAX if cv else 4
    for extra in (dict(), dict(nonneg=(True, True), center=True), dict(L1=(0.02, 0.02))):
        a = R.reg_deflation_svd(A, k, stored=keep, **kw, **extra)
        b = C.cv_deflation_svd(A, k, stored=keep, **kw, **extra)
        for key in ("u", "d", "v", "iters", "test_loss"):
            assert np.array_equal(a[key], b[key]), key
        assert (a["k_selected"], a["k_computed"], a["n_test"], a["frob"]) == (b["k_selected"], b["k_computed"], b["n_test"], b["frob"])


def small():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(9)
    F = np.linalg.qr(rng.standard_normal((9, 4)))[0]
    L = np.where(rng.random((9, 9)) < 0.4, rng.standard_normal((9, 9)), 0.0)          # non-symmetric
    rows, cols = np.nonzero(L)
    o = np.lexsort((rows, cols))
    return x, F, L, (rows[o], cols[o], L[rows[o], cols[o]], 9)


def brute_chain(x, L1, L2, nonneg, ub, nsq):
    out = []
    for v in x:
        if L2 > 0:
            v = v * (1.0 / (1.0 + L2 / nsq))
        if L1 > 0:
            th = L1 / (2.0 * nsq)
            v = v - th if v > th else (v + th if v < -th else 0.0)
        if nonneg:
            v = max(v, 0.0)
        if ub > 0:
            v = min(v, ub)
        out.append(v)
    return np.array(out)


def test_l21_takes_the_norm_before_the_shrink_and_keeps_the_guard():
    x, F, L, g = small()
    nsq = 0.8
    norm = 0.0
    for v in x:
        norm += v * v
    norm = norm ** 0.5
    want = brute_chain(x, 0.1, 0.05 + 0.3 / norm, True, 0.9, nsq)
    got = R.reg_side(x, F[:, :0], nsq, 0.1, 0.05, True, 0.9, 0.3, 0.0, None, 0.0)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    after = brute_chain(x, 0.1, 0.05, True, 0.9, nsq)                     # the norm after the element chain gives another vector
    wrong = brute_chain(x, 0.1, 0.05 + 0.3 / np.linalg.norm(after), True, 0.9, nsq)
    assert np.max(np.abs(wrong - want)) > 1e-3
    tiny = x * 1e-12                                                     # |x| <= 1e-10: L21 adds nothing
    assert np.array_equal(R.reg_side(tiny, F[:, :0], nsq, 0.0, 0.05, False, 0.0, 0.3, 0.0, None, 0.0),
                          R.reg_side(tiny, F[:, :0], nsq, 0.0, 0.05, False, 0.0, 0.0, 0.0, None, 0.0))
    assert R.l21_l2(tiny, 0.05, 0.3) == 0.05 and R.l21_l2(x.astype(np.float32), 0.05, 0.3).dtype == np.float32


def test_angular_against_an_element_loop_and_its_no_op_at_k0():
    x, F, L, g = small()
    nsq, ang = 0.8, 0.25
    want = x.copy()
    dots = [sum(F[i, q] * x[i] for i in range(9)) for q in range(4)]
    for i in range(9):
        want[i] -= (ang / nsq) * sum(F[i, q] * dots[q] for q in range(4))
    assert np.allclose(R.angular_step(x, F, ang, nsq), want, rtol=1e-13, atol=1e-15)
    assert R.angular_step(x, F[:, :0], ang, nsq) is x and R.angular_step(x, F, 0.0, nsq) is x
    # in the chain F' x is taken after the element chain
    z = R.reg_side(x, F, nsq, 0.0, 0.0, True, 0.0, 0.0, ang, None, 0.0)
    xp = np.maximum(x, 0)
    assert np.allclose(z, xp - (ang / nsq) * (F @ (F.T @ xp)), rtol=1e-13, atol=1e-15)


def test_graph_is_l_x_not_l_transpose_x_and_runs_after_angular():
    x, F, L, g = small()
    nsq, lam = 0.8, 0.03
    want = x.copy()
    for i in range(9):
        want[i] -= (lam / nsq) * sum(L[i, j] * x[j] for j in range(9))
    got = R.graph_step(x, g, lam, nsq)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-15)
    assert np.max(np.abs(got - (x - (lam / nsq) * (L.T @ x)))) > 1e-3
    assert np.allclose(R.graph_matvec(g, x), L @ x, rtol=1e-13, atol=1e-15)
    y = R.angular_step(x, F, 0.2, nsq)
    assert np.allclose(R.reg_side(x, F, nsq, 0, 0, False, 0, 0, 0.2, g, lam), y - (lam / nsq) * (L @ y), rtol=1e-13, atol=1e-15)
    zero = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), 9)
    assert np.array_equal(R.graph_step(x, zero, lam, nsq), x)                       # L = 0: the identity


def test_graph_helpers():
    g = R.ring_laplacian(12, 1)
    L = R.graph_dense(g)
    assert np.allclose(L, L.T) and np.allclose(L.sum(axis=1), 0) and np.all((L != 0).sum(axis=1) == 5)
    gs = R.ring_laplacian(12, 1, skew=True)
    Ls = R.graph_dense(gs)
    assert not np.allclose(Ls, Ls.T) and np.allclose(Ls.sum(axis=1), 0)
    for gg in (g, gs):
        assert np.max(np.abs(np.linalg.eigvals(R.graph_dense(gg)))) <= R.lambda_max_bound(gg) * (1 + 1e-12)
        p, i, x, dim, lam = R.graph_csc(gg, 0.5)
        assert np.array_equal(sp.csc_matrix((x, i, p), shape=(dim, dim)).toarray(), R.graph_dense(gg))


def test_angular_on_an_unconstrained_fit_shrinks_the_overlap_with_the_stored_factors():
    A, keep = R.shape_input("sparse130x67")
    kw = dict(tol=0.0, maxit=6, seed=5)
    plain = R.reg_deflation_svd(A, 2, stored=keep, **kw)
    U1, V1 = plain["u"][:, :1], plain["v"][:, :1]
    nsq = 1.0
    rng = np.random.default_rng(0)
    for F in (U1, V1):
        x = rng.standard_normal(F.shape[0])
        assert np.linalg.norm(F.T @ R.angular_step(x, F, 0.3, nsq)) < np.linalg.norm(F.T @ x)
    # and in the loop: the raw second factor overlaps the first less with angular on (both before the final Gram-Schmidt would hide it)
    ang = R.reg_deflation_svd(A, 2, stored=keep, angular=(0.5, 0.5), **kw)
    assert ang["iters"].tolist() == plain["iters"].tolist() and not np.array_equal(ang["u"][:, 1], plain["u"][:, 1])


# ------------------------------------------------------------------------------------------------ cases
def test_measured_covers_every_case_and_is_not_below_the_recomputed_deviation():
    assert set(R.MEASURED) == set(R.CASES)
    for s, p in R.CASES:
        dev = R.deviation(R.case_ref(s, p, np.float32), R.case_ref(s, p, np.float64))
        assert dev <= R.MEASURED[(s, p)], (s, p, dev)
        assert R.MEASURED[(s, p)] <= 5e-4, (s, p)               # the regularisers keep float32 within 5e-4 of float64


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%s" % c)
def test_parity_cases_never_come_within_100_eps_of_convergence(case):
    """tol = 0 ends a factor only on a rounded-negative distance; 100 eps of room keeps the fixed iteration count the same in the
    restatement and on the device, in both precisions."""
    for dt in (np.float32, np.float64):
        r = R.case_ref(*case, dt)
        assert r["k_computed"] >= 4 and np.all(r["iters"] == R.case_iters(*case))
        for d in r["dist"]:
            assert len(d) == R.case_iters(*case) and min(d) > 100 * np.finfo(dt).eps, (dt, min(d))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-%s" % c)
def test_float64_restatement_is_within_1e11_of_longdouble(case):
    a, b = R.case_ref(*case, np.float64), R.case_ref(*case, np.longdouble)
    assert np.array_equal(a["iters"], b["iters"]) and a["k_selected"] == b["k_selected"]
    assert R.deviation(a, b) < 1e-11
    if a["test_loss"].size:
        tl = b["test_loss"].astype(np.float64)
        assert np.all(np.abs(a["test_loss"] - tl) < 1e-11 * tl)


def test_graph_lambdas_stay_clear_of_the_amplifying_range():
    for s in R.SHAPES:
        for skew in (False, True):
            gu, gv, lu, lv = R.shape_graphs(s, skew)
            assert lu * R.lambda_max_bound(gu) <= 0.4 and lv * R.lambda_max_bound(gv) <= 0.4


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_convergence_cases_stop_clear_of_their_tolerance(dt):
    A, keep, kw = R.convergence_kwargs(dt)
    r = R.reg_deflation_svd(A, R.K, stored=keep, dtype=dt, **kw)
    assert r["k_computed"] == R.K and np.all(r["iters"] < 200) and np.all(r["iters"] >= 2)
    for f, d in enumerate(r["dist"]):
        tk = R.tol_k_of(r["d"], f, kw["tol"], dt)
        assert len(d) == r["iters"][f] and d[-1] < tk / 2 and d[-2] > 2 * tk, (f, d[-2:], tk)


# ------------------------------------------------------------------------------------------------ surface
LAP = sp.csc_matrix(R.graph_dense(R.ring_laplacian(40, 1)))


@pytest.mark.parametrize("kw, msg", [
    (dict(L21=-1), "L21 penalties must be non-negative"),
    (dict(L21=(0, -0.1)), "L21 penalties must be non-negative"),
    (dict(angular=(-0.5, 0)), "angular penalties must be non-negative"),
    (dict(graph_lambda=-0.1), "graph_lambda must be non-negative"),
    (dict(graph_U=np.eye(60)), "graph_U must be a sparse matrix"),
    (dict(graph_V=np.eye(40)), "graph_V must be a sparse matrix"),
    (dict(graph_U=LAP, graph_lambda=0.1), "graph_U must be 60 x 60 (matching rows of A)"),
    (dict(graph_V=sp.csc_matrix((60, 60)), graph_lambda=0.1), "graph_V must be 40 x 40 (matching columns of A)"),
    (dict(angular=0.1, method="lanczos"), "method 'lanczos' does not support Gram-level regularization (angular/graph). Use 'krylov'."),
    (dict(graph_V=LAP, graph_lambda=(0, 0.1), method="randomized"),
     "method 'randomized' does not support Gram-level regularization (angular/graph). Use 'krylov'."),
    (dict(L21=0.1, method="irlba"), "method 'irlba' does not support constraints (L1/L2/nonneg/bounds/L21). Use 'deflation' or 'krylov'."),
])
def test_surface_raises_rs_messages_before_any_device_work(kw, msg):
    from rcppml_amd import svd as S
    with pytest.raises(ValueError) as e:
        S.svd(C.dense_input(), k=3, **kw)
    assert str(e.value) == msg


def test_routing_table():
    from rcppml_amd import _abi, svd as S
    rm = lambda k, method="auto", **kw: S.resolve_method(k, method, **kw)[0]
    assert rm(6, angular=0.1) == "deflation" and rm(8, angular=0.1) == "krylov"
    assert rm(6, L21=(0, 0.1)) == "deflation" and rm(8, L21=0.1) == "krylov"
    assert rm(6, graph_lambda=0.1, graph=(False, True)) == "deflation" and rm(8, graph_lambda=0.1, graph=(True, False)) == "krylov"
    assert rm(8, graph_lambda=(0.1, 0), graph=(False, True)) == "lanczos"           # a graph whose side has lambda 0 is not active
    assert rm(8, graph_lambda=0.1) == "lanczos"                                     # nor is a lambda without a graph
    assert rm(8) == "lanczos" and rm(6, nonneg=True) == "deflation"                 # calls without the new arguments go where they went
    assert S.resolve_cv(10, test_fraction=0.1, angular=0.1)[1] == "krylov" and S.resolve_cv(5, test_fraction=0.1, L21=0.1)[1] == "deflation"
    assert S.resolve_cv(10, test_fraction=0.1) == (10, "deflation", 0.1, False)
    A = C.dense_input()
    for kw in (dict(k=8, angular=0.1), dict(k=3, method="krylov", L21=0.1), dict(k=8, graph_V=LAP, graph_lambda=0.1),
               dict(k="auto", k_max=9, angular=0.1)):
        with pytest.raises(_abi.BackendError) as e:                                 # raised before any device work
            S.svd(A, **kw)
        assert 'method = "deflation"' in str(e.value), kw


def test_routing_sends_deflation_with_a_term_on_to_svd_reg(monkeypatch):
    from rcppml_amd import _abi, svd as S
    seen = []

    def fake(name):
        def f(src, k, **kw):
            seen.append((name, k, kw))
            raise _abi.BackendError("stop here")
        return f
    for name in ("svd_reg", "svd_cv", "svd_pca", "svd_krylov"):
        monkeypatch.setattr(_abi, name, fake(name))
    A = C.dense_input()
    calls = [dict(k=6, angular=0.1), dict(k=3, method="deflation", L21=(0.1, 0.2)), dict(k=3, graph_V=LAP, graph_lambda=(0.5, 0.02)),
             dict(k="auto", k_max=6, L21=0.1), dict(k=3, angular=0.1, mask=sp.csc_matrix(A > 40)),
             dict(k=3, graph_V=LAP, graph_lambda=0), dict(k=3, test_fraction=0.1), dict(k=3, nonneg=True)]
    for kw in calls:
        with pytest.raises(_abi.BackendError):
            S.svd(A, **kw)
    assert [s[0] for s in seen] == ["svd_reg"] * 5 + ["svd_pca", "svd_cv", "svd_pca"]
    assert seen[1][2]["L21"].tolist() == [0.1, 0.2] and seen[1][2]["graph_u"] is None
    gv = seen[2][2]["graph_v"]
    assert seen[2][2]["graph_u"] is None and gv[3] == 40 and gv[4] == 0.02 and len(gv[0]) == 41      # no graph_U: lambda[0] is unused
    assert seen[3][2]["test_fraction"] == 0.05 and seen[4][2]["obs_mask"] is not None


# ------------------------------------------------------------------------------------------------ entries
def test_header_declares_the_reg_entries_and_abi_binds_them():
    from rcppml_amd import _abi
    src = open(os.path.join(os.path.dirname(HERE), "include", "rcppml_gpu.h")).read()
    for name, count in (("rcppml_gpu_svd_reg_ex", 58), ("rcppml_gpu_svd_reg_dense_ex", 55)):
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert m.group(1).count("*") == count and len(m.group(1).split(",")) == count, name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(_abi.lib(), name), name
    # the cv entry's parameters in order, the new ones after ub_v
    names = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % n, src, flags=re.S).group(1).split(",")]
    cv, reg = names("rcppml_gpu_svd_cv_ex"), names("rcppml_gpu_svd_reg_ex")
    at = reg.index("ub_v") + 1
    assert reg[:at] + reg[at + 16:] == cv
    assert reg[at:at + 4] == ["L21_u", "L21_v", "angular_u", "angular_v"]
    assert reg[at + 4:at + 16] == ["graph_%s_%s" % (s, w) for s in "uv" for w in ("p", "i", "x", "dim", "nnz", "lambda")]


def _csc(A):
    S = sp.csc_matrix(A)
    S.sort_indices()
    return (S.indptr, S.indices, S.data, A.shape[0], A.shape[1])


def _graph(dim, lam=0.1, **edit):
    p, i, x, d, lam = R.graph_csc(R.ring_laplacian(dim, 1), lam)
    g = dict(p=p.copy(), i=i.copy(), x=x.copy(), dim=d, lam=lam)
    for key, (pos, val) in edit.items():
        g[key][pos] = val
    return (g["p"], g["i"], g["x"], g["dim"], g["lam"])


@pytest.mark.parametrize("kw, word", [
    (dict(L21=(-0.1, 0)), "L21"),
    (dict(L21=(0, float("nan"))), "L21"),
    (dict(angular=(0, -1.0)), "angular"),
    (dict(angular=(float("inf"), 0)), "angular"),
    (dict(graph_u=_graph(60, lam=-0.5)), "graph_u lambda"),
    (dict(graph_v=_graph(40, lam=float("nan"))), "graph_v lambda"),
    (dict(graph_u=_graph(40)), "graph_u must be 60 x 60"),                              # dim != m
    (dict(graph_v=_graph(60)), "graph_v must be 40 x 40"),
    (dict(graph_u=_graph(60, p=(0, 1))), "malformed graph_u CSC"),
    (dict(graph_v=_graph(40, i=(3, 40))), "malformed graph_v CSC"),                            # row out of range
    (dict(graph_v=_graph(40, x=(7, float("nan")))), "non-finite"),
    (dict(patience=0, L21=(0.1, 0.1)), "patience"),                                     # what the cv entries refuse
    (dict(k=41, angular=(0.1, 0.1)), "k_max"),
])
def test_reg_entry_refusals_leave_buffers_untouched(kw, word):
    """Refused before any device work, so these hold with or without a GPU."""
    from rcppml_amd import _abi
    A = C.dense_input()
    kw = dict(kw)
    k = kw.pop("k", 3)
    for dense, prec in ((False, "double"), (True, "float")):
        bufs = dict(U=np.full(60 * k, 7.0), d=np.full(k, 7.0), V=np.full(40 * k, 7.0), row_means=np.full(60, 7.0),
                    iters=np.full(k, 7, np.int32), test_loss=np.full(k, 7.0))
        args = dict(dict(test_fraction=0.1, center=True), **kw)
        r = _abi.svd_reg(A if dense else _csc(A), k, dense=dense, precision=prec, buffers=bufs, **args)
        assert r["status"] == -1 and word in r["error"], r["error"]
        assert all(np.all(b == 7) for b in bufs.values())
        assert (r["k"], r["k_computed"], r["n_test"], r["n_masked"], r["frob"], r["wall_ms"]) == (0, 0, 0, 0, 0.0, 0.0)


def test_the_reference_entries_still_refuse_the_three_terms():
    from rcppml_amd import _abi
    A = C.dense_input()
    for kw, word in ((dict(L21=(0.1, 0)), "L21"), (dict(angular=(0, 0.1)), "angular"), (dict(graph_v=_graph(40)), "graph")):
        r = _abi.svd_pca(A, 3, dense=True, **kw)
        assert r["status"] == -1 and word in r["error"]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud():
    from rcppml_amd import _abi, svd
    with pytest.raises(_abi.BackendError):
        svd.svd(C.dense_input(), k=3, L21=0.1)
    r = _abi.svd_reg(C.dense_input(), 3, dense=True, angular=(0.1, 0.1))
    assert r["status"] == -1 and r["error"]
