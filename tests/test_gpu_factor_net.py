"""GPU checks of the factor-graph path (rcppml_amd/csrc/ops_graph.hip, kernels_graph.hip.h, rcppml_amd/factor_net.py) against the numpy
restatement (tests/factor_net_ref.py).

Tolerance.  Device and restatement differ in summation order only, amplified by the solves.  For every input
the restatement is run twice -- as written, and with every contraction visited in reverse order and accumulated in long double --
and delta is the largest factor_net_ref.rel_diff over the outputs.  The device gets 100 * max(delta, 2^-52).  delta never sees the
device result (tests/test_factor_net_cpu.py keeps it at or under 1e-8 on every input used here).  Every case prints delta and the
device's deviation.  The assembly op is a copy (concat) or the same fp64 additions in the same order (add): it must be exact.
"""
import numpy as np
import pytest
import torch

import factor_net_inputs as I
import factor_net_ref as F
from rcppml_amd import _abi
from rcppml_amd import factor_net as fn
from rcppml_amd import nmf as N
from rcppml_amd.data import CSC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _abi.Context(0)
    yield c
    c.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


# ------------------------------------------------------------------------------------------------------------------ assemble op
CONCAT_RANKS = [(1,), (64,), (128,), (1, 3), (17, 64), (128, 1), (3, 128), (1, 3, 17), (64, 128, 3)]
ADD_RANKS = [(k,) * r for k in (1, 3, 17, 64, 128) for r in (2, 3)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 700])
def test_assemble_is_exact(ctx, n, mode):
    rng = np.random.default_rng(1000 * n + mode)
    for ranks in (ADD_RANKS if mode else CONCAT_RANKS):
        for p in (0, 1, 2):
            Hs = [rng.standard_normal((k, n)) for k in ranks]
            Z = rng.standard_normal((p, n)) if p else None
            if mode:
                S = Hs[0].copy()
                for Hb in Hs[1:]:
                    S = S + Hb
            parts = [S.T] if mode else [Hb.T for Hb in Hs]
            want = np.concatenate(parts + ([Z.T] if p else []), axis=1)                  # n x c
            c = want.shape[1]
            X = torch.full((c, n), -7.0, dtype=torch.float64, device="cuda")             # (c, n) row-major = column-major n x c
            ctx.graph_assemble(mode, [dev(Hb.T) for Hb in Hs], ranks, n, dev(Z.T) if p else None, p, X)
            ctx.sync()
            assert np.array_equal(X.cpu().numpy().T, want), (ranks, p)


# ---------------------------------------------------------------------------------------------------------------------- loss op
@pytest.mark.parametrize("k", [1, 2, 16, 33, 128])
def test_layer_loss_parity_and_repeatability(ctx, k):
    rng = np.random.default_rng(k)
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    for c in (1, 5, 48, 130):
        for rows in (1, 257, 1000):
            W, d, H = rng.uniform(0, 1, (rows, k)), rng.uniform(0.5, 2, k), rng.uniform(0, 1, (k, c))
            X = W @ (d[:, None] * H) + 0.1 * rng.standard_normal((rows, c))
            ref = F.layer_loss(X, W, d, H)
            delta = F.rel_diff(F.layer_loss(X, W, d, H, variant=True), ref)
            dX, dW, dd, dH = dev(X.T), dev(W), dev(d), dev(H.T)
            scale = 1.0 / (rows * c)
            ctx.graph_layer_loss(dX, rows, c, dW, dd, dH, k, scale, out[0:])
            ctx.graph_layer_loss(dX, rows, c, dW, dd, dH, k, scale, out[1:])
            ctx.sync()
            got = out.cpu().numpy()
            err = F.rel_diff(got[0], ref)
            print("layer loss k=%d c=%d rows=%d: delta %.3e device %.3e bound %.3e" % (k, c, rows, delta, err, I.bound(delta)))
            assert got[0] == got[1]
            assert err <= I.bound(delta)


# -------------------------------------------------------------------------------------------------- the entry against the restatement
def run_entry(dname, g, **kw):
    csc, dense = I.data(dname)
    m, n = dense.shape
    args = ((csc[0], csc[1], csc[2]), None) if csc is not None else (None, dense)
    return _abi.factor_net_fit(args[0], args[1], m, n, **I.abi_graph(g), **kw)


def deviation(r, ref):
    got = dict(layers=r["layers"], layer_loss=r["layer_loss"], loss=r["loss"])
    return max(F.rel_diff(a, b) for a, b in zip(F.outputs(got), F.outputs(ref)))


@pytest.mark.parametrize("case", [c[0] for c in I.STEP_CASES])
def test_one_outer_step_from_supplied_states(case):
    _, dname, _, solver, norm = next(c for c in I.STEP_CASES if c[0] == case)
    g, states, ref, delta = I.step_reference(case)
    r = run_entry(dname, g, max_iter=1, tol=0.0, solver_mode=solver, norm_type=norm, states=states)
    assert r["status"] == 0, r["error"]
    err = deviation(r, ref)
    print("step %s: delta %.3e device %.3e bound %.3e" % (case, delta, err, I.bound(delta)))
    assert r["iter"] == 1 and not r["converged"]
    assert err <= I.bound(delta)


@pytest.mark.parametrize("case", [c[0] for c in I.FIT_CASES])
def test_full_fit_with_warm_up(case):
    _, dname, _, solver, max_iter, tol = next(c for c in I.FIT_CASES if c[0] == case)
    g, ref, delta = I.fit_reference(case)
    r = run_entry(dname, g, max_iter=max_iter, tol=tol, seed=I.SEED, solver_mode=solver, norm_type=0)
    assert r["status"] == 0, r["error"]
    err = deviation(r, ref)
    print("fit %s: delta %.3e device %.3e bound %.3e iterations %d" % (case, delta, err, I.bound(delta), r["iter"]))
    assert r["iter"] == ref["iter"] and r["converged"] == ref["converged"]
    assert err <= I.bound(delta)
    if tol == 0.5:
        # the loop stopped on the convergence test: total_loss is the PREVIOUS iteration's, not the sum of the last layer losses
        assert r["converged"] and r["iter"] == 2 and r["loss"] != float(np.sum(r["layer_loss"]))


def test_repeatable_bitwise():
    g = I.graph("concat", 1183)
    a = run_entry("hawaiibirds", g, max_iter=2, tol=0.0, seed=3, solver_mode=0, norm_type=0)
    b = run_entry("hawaiibirds", g, max_iter=2, tol=0.0, seed=3, solver_mode=0, norm_type=0)
    assert a["status"] == 0 and b["status"] == 0
    assert all(np.array_equal(x, y) for x, y in zip(F.outputs(a), F.outputs(b)))


# ---------------------------------------------------------------------------------------------------------------------- surface
def hawaii_csc():
    (p, i, x, shape), _ = I.data("hawaiibirds")
    return CSC(shape, p, i, x)


def test_single_layer_fit_is_nmf():
    A = hawaii_csc()
    cfg = fn.factor_config(maxit=8, tol=1e-5, seed=11, norm="L2", precision="fp64")
    x = fn.factor_input(A, "birds")
    res = fn.fit(fn.factor_net(x, fn.nmf_layer(x, 6, L1=0.01, H=fn.H(L2=0.05)), cfg))
    mod = N.nmf(A, 6, tol=1e-5, maxit=8, seed=11, norm="L2", solver="cholesky", L1=(0.01, 0.01), L2=(0.0, 0.05), precision="fp64")
    L = res["L1"]
    assert np.array_equal(L.W, mod.w) and np.array_equal(L.d, mod.d) and np.array_equal(L.H, mod.h)
    assert res.n_layers == 1 and not res.multi_modal and res.total_iterations == mod.misc["iter"] and res.total_loss == mod.misc["loss"]
    new = A.to_scipy().toarray()[:, :50]
    assert np.array_equal(fn.predict(res, new), N.predict(mod, new))


def test_shared_fit_is_nmf_on_the_stack():
    dense = hawaii_csc().to_scipy().toarray()
    import scipy.sparse as sp
    parts = [dense[:100], dense[100:]]
    cfg = fn.factor_config(maxit=5, seed=5, precision="fp64")
    ins = [fn.factor_input(CSC.from_scipy(sp.csc_matrix(parts[0])), "top"), fn.factor_input(CSC.from_scipy(sp.csc_matrix(parts[1])))]
    res = fn.fit(fn.factor_net(ins, fn.nmf_layer(fn.factor_shared(*ins), 4), cfg))
    mod = N.nmf(CSC.from_scipy(sp.csc_matrix(dense)), 4, maxit=5, seed=5, solver="cholesky", precision="fp64")
    L = res.L1
    assert res.multi_modal and res.input_names == ["top", "input2"] and list(L.W) == ["top", "input2"]
    assert np.array_equal(L.W["top"], mod.w[:100]) and np.array_equal(L.W["input2"], mod.w[100:])
    assert np.array_equal(L.d, mod.d) and np.array_equal(L.H, mod.h)


def test_deep_fit_is_the_raw_entry():
    A = hawaii_csc()
    x = fn.factor_input(A)
    a, b = fn.nmf_layer(x, 5), fn.nmf_layer(x, 3, H=fn.H(L1=0.01))
    top = fn.svd_layer(fn.factor_condition(fn.factor_concat(a, b), I.cond_block(1183, transposed=True)), 4, name="top")
    res = fn.fit(fn.factor_net(x, top, fn.factor_config(maxit=2, seed=9, solver="cd", norm="L2")))
    g = [F.layer(5), F.layer(3, L1=(0.0, 0.01)), F.layer(4, "concat", [0, 1], Z=I.cond_block(1183), nonneg=(False, False))]
    r = run_entry("hawaiibirds", g, max_iter=2, tol=1e-4, seed=9, solver_mode=0, norm_type=1)
    assert r["status"] == 0, r["error"]
    assert list(res.layers) == ["L1", "L2", "top"] and res.n_layers == 3 and not res.multi_modal
    for name, (Wm, dv, Hm) in zip(res.layers, r["layers"]):
        L = res[name]
        assert np.array_equal(L.W, Wm) and np.array_equal(L.d, dv) and np.array_equal(L.H, Hm)
        assert L.iterations == r["iter"] and L.loss == r["loss"]
    assert res.total_loss == r["loss"] and res.total_iterations == r["iter"] == 2 and np.array_equal(res.layer_losses, r["layer_loss"])
    assert res.top.H.shape == (4, 10)          # 5 + 3 branch columns and the p = 2 condition columns


def test_a_refused_call_writes_nothing():
    g = I.graph("chain", 1183)
    for change, kw, word in ((dict(k=129), {}, "rank must be in"), (dict(k=65), dict(solver_mode=1), "Cholesky solver needs a rank <= 64"),
                             (dict(br=[1]), {}, "a branch must be an earlier layer"), ({}, dict(max_iter=0), "max_iter must be >= 1"),
                             ({}, dict(norm_type=5), "norm_type")):
        bad = [dict(l) for l in g]
        bad[1].update(change)
        args = dict(max_iter=2, tol=0.0, solver_mode=0, norm_type=0)
        args.update(kw)
        r = run_entry("hawaiibirds", bad, **args)
        assert r["status"] == -1 and word in r["error"], r["error"]
        Wb, db, Hb, ll, it, conv, loss = r["buffers"]
        assert np.all(Wb == -7) and np.all(db == -7) and np.all(Hb == -7) and np.all(ll == -7)
        assert (it, conv, loss) == (-7, -7, -7.0)
    with pytest.raises(_abi.BackendError, match="Cholesky solver needs a rank <= 64"):
        x = fn.factor_input(np.random.default_rng(0).uniform(size=(90, 80)))
        fn.fit(fn.factor_net(x, fn.nmf_layer(fn.nmf_layer(x, 70), 2), fn.factor_config(maxit=1)))
