"""CPU checks of the factor-graph surface (rcppml_amd/factor_net.py) and of its numpy restatement (tests/factor_net_ref.py): the
restatement is pinned to the project's CPU oracle, the topology / naming / validation / refusal rules are checked message for
message, and every input of the GPU parity tests is checked for a summation-order sensitivity at or under 1e-8."""
import os

import numpy as np
import pytest

import factor_net_inputs as I
import factor_net_ref as F
from oracle import oracle as O
from rcppml_amd import _abi
from rcppml_amd import factor_net as fn
from rcppml_amd.data import CSC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hawaii():
    (p, i, x, shape), dense = I.data("hawaiibirds")
    return O.Csc(shape, p, i, x), dense


# ------------------------------------------------------------------------------------------- the restatement against the oracle
@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("dense_input", [False, True])
def test_step_equals_the_oracle(dense_input, solver, norm):
    """One iteration from W (max_iter = 1, sort_model = False): on the sparse matrix through the oracle's standard path (the sums run
    over the nonzeros) and on dense_input = True.  Restatement and oracle differ in summation order only; the bound is the
    restatement's own delta rule."""
    A, dense = hawaii()
    m, n = dense.shape
    k = 8
    g = F.layer(k, L1=(0.01, 0.02), L2=(0.0, 0.1), ub=(0.0, 0.5))
    W0, H0 = F.init_factors(43, k, m, n)
    ref = F.iterate(dense, W0, H0, g, solver=solver, norm=norm)
    var = F.iterate(dense, W0, H0, g, solver=solver, norm=norm, variant=True)
    delta = max(F.rel_diff(a, b) for a, b in zip(var, ref))
    r = O.nmf_fit(O.dense_as_csc(dense) if dense_input else A, W0, np.ascontiguousarray(H0.T), max_iter=1, tol=0.0, L1=g["L1"], L2=g["L2"],
                  ub=g["ub"], solver_mode=solver, norm_type=norm, sort_model=False, dense_input=dense_input, unfused=not dense_input)
    dev = max(F.rel_diff(a, b) for a, b in zip((r.W_T, r.d, r.H.T), ref))
    print("step dense=%d solver=%d norm=%d: delta %.3e oracle %.3e" % (dense_input, solver, norm, delta, dev))
    assert dev <= I.bound(delta)


@pytest.mark.parametrize("solver", [0, 1])
def test_warm_up_equals_the_oracle(solver):
    A, dense = hawaii()
    m, n = dense.shape
    k, seed_base, i = 8, 42, 2
    Wo, Ho = O.init_factors(seed_base + i, k, m, n)
    W0, H0 = F.init_factors(seed_base + i, k, m, n)
    assert np.array_equal(Wo, W0) and np.array_equal(Ho, H0.T)
    g = F.layer(k)
    ref = F.warm_up(dense, g, seed_base + i, 10, 1e-4, solver=solver)
    var = F.warm_up(dense, g, seed_base + i, 10, 1e-4, solver=solver, variant=True)
    delta = max(F.rel_diff(a, b) for a, b in zip(var[:3], ref[:3]))
    r = O.nmf_fit(O.dense_as_csc(dense), Wo, Ho, max_iter=10, tol=1e-4, solver_mode=solver, sort_model=False, dense_input=True)
    dev = max(F.rel_diff(a, b) for a, b in zip((r.W_T, r.d, r.H.T), ref[:3]))
    print("warm-up solver=%d: delta %.3e oracle %.3e iterations %d / %d" % (solver, delta, dev, ref[3], r.iter))
    assert ref[3] == r.iter and dev <= I.bound(delta)


def test_warm_up_stops_on_the_fits_convergence_rule():
    """tol = 0.5: every check converges, patience 5 is reached at the sixth iteration -- in the restatement and in the oracle."""
    _, dense = hawaii()
    m, n = dense.shape
    Wo, Ho = O.init_factors(44, 4, m, n)
    ref = F.warm_up(dense, F.layer(4), 44, 10, 0.5)
    r = O.nmf_fit(O.dense_as_csc(dense), Wo, Ho, max_iter=10, tol=0.5, solver_mode=1, sort_model=False, dense_input=True)
    assert ref[3] == r.iter == 6
    assert max(F.rel_diff(a, b) for a, b in zip((r.W_T, r.d, r.H.T), ref[:3])) <= 1e-10


def test_total_loss_is_the_previous_iterations_on_convergence():
    g, ref, _ = I.fit_reference("fit-chain-tol0.5")
    assert ref["converged"] and ref["iter"] == 2
    assert ref["loss"] != float(ref["layer_loss"].sum())
    _, dense = hawaii()
    one = F.fit_deep(dense, g, max_iter=1, tol=0.5, seed=I.SEED)             # max_iter = 1: the warm-up runs one iteration only
    assert not one["converged"] and one["loss"] == float(np.sum(one["layer_loss"]))


@pytest.mark.parametrize("case", [c[0] for c in I.STEP_CASES])
def test_step_inputs_are_not_order_sensitive(case):
    delta = I.step_reference(case)[3]
    print("%s: delta %.3e" % (case, delta))
    assert delta <= I.DELTA_MAX


@pytest.mark.parametrize("case", [c[0] for c in I.FIT_CASES])
def test_fit_inputs_are_not_order_sensitive(case):
    delta = I.fit_reference(case)[2]
    print("%s: delta %.3e" % (case, delta))
    assert delta <= I.DELTA_MAX


# ------------------------------------------------------------------------------------------------------------ topology, naming
def small(m=12, n=9, seed=1):
    return np.random.default_rng(seed).uniform(0, 1, (m, n))


def test_chain_names_and_descriptor():
    x = fn.factor_input(small(), "X")
    l1 = fn.nmf_layer(x, 4)
    l2 = fn.nmf_layer(l1, 3, name="mid")
    l3 = fn.svd_layer(l2, 2)
    net = fn.factor_net(x, l3)
    assert net.layer_names == ["L1", "mid", "L3"] and net.n_layers == 3
    d = fn.deep_descriptor(net)
    assert d["rank"] == [4, 3, 2] and d["src_kind"] == [0, 1, 1] and d["branches"] == [[], [0], [1]]
    assert d["nonneg"] == [(True, True), (True, True), (False, False)]
    assert _abi.factor_net_dims(12, 9, d["rank"], d["src_kind"], d["branches"], [0, 0, 0]) == [(12, 9), (9, 4), (4, 3)]


def test_two_branches_into_concat_and_add():
    x = fn.factor_input(small())
    a, b = fn.nmf_layer(x, 5), fn.nmf_layer(x, 3)
    net = fn.factor_net(x, fn.nmf_layer(fn.factor_concat(a, b), 4))
    assert net.layer_names == ["L1", "L2", "L3"] and net.layers[0] is a and net.layers[1] is b          # branches in argument order
    d = fn.deep_descriptor(net)
    assert d["src_kind"] == [0, 0, 2] and d["branches"] == [[], [], [0, 1]]
    assert _abi.factor_net_dims(12, 9, d["rank"], d["src_kind"], d["branches"], [0, 0, 0])[2] == (9, 8)
    c, e = fn.nmf_layer(x, 4), fn.nmf_layer(x, 4)
    d = fn.deep_descriptor(fn.factor_net(x, fn.nmf_layer(fn.factor_add(e, c), 2)))
    assert d["src_kind"] == [0, 0, 3] and d["branches"] == [[], [], [0, 1]]
    assert _abi.factor_net_dims(12, 9, d["rank"], d["src_kind"], d["branches"], [0, 0, 0])[2] == (9, 4)


@pytest.mark.parametrize("transposed", [False, True])
def test_condition_orientation(transposed):
    x = fn.factor_input(small())
    Z = I.cond_block(9, transposed)                      # p x n, or n x p
    l1 = fn.nmf_layer(x, 4)
    d = fn.deep_descriptor(fn.factor_net(x, fn.nmf_layer(fn.factor_condition(l1, Z), 2)))
    assert d["cond_Z"][0] is None and np.array_equal(d["cond_Z"][1], I.cond_block(9))
    a, b = fn.nmf_layer(x, 3), fn.nmf_layer(x, 2)
    d = fn.deep_descriptor(fn.factor_net(x, fn.nmf_layer(fn.factor_condition(fn.factor_concat(a, b), Z), 2)))
    assert d["src_kind"][2] == 2 and np.array_equal(d["cond_Z"][2], I.cond_block(9))
    with pytest.raises(ValueError, match="Conditioning Z dimension mismatch"):
        fn.deep_descriptor(fn.factor_net(x, fn.nmf_layer(fn.factor_condition(l1, np.ones((5, 4))), 2)))
    assert fn.orient_Z(np.ones((9, 9)), 9).shape == (9, 9)          # square: taken as p x n


def test_solver_rule_and_inheritance():
    assert fn.solver_mode(fn.factor_config()) == 1                               # auto: Cholesky for MSE
    assert fn.solver_mode(fn.factor_config(loss="gp")) == 0
    assert fn.solver_mode(fn.factor_config(solver="cd")) == 0
    assert fn.solver_mode(fn.factor_config(solver="cholesky", loss="nb")) == 1
    x = fn.factor_input(small())
    w, h = fn.factor_settings(fn.nmf_layer(x, 3, L1=0.1, L2=0.2, W=fn.W(L1=0.3, nonneg=False), H=fn.H(upper_bound=2.0)))
    assert (w["L1"], h["L1"], w["L2"], h["L2"]) == (0.3, 0.1, 0.2, 0.2)
    assert (w["nonneg"], h["nonneg"], w["upper_bound"], h["upper_bound"]) == (False, True, 0, 2.0)
    w, h = fn.factor_settings(fn.svd_layer(x, 3, H=fn.H(nonneg=True)))
    assert (w["nonneg"], h["nonneg"]) == (False, True)


# ----------------------------------------------------------------------------------------------------- validation, message by message
def test_constructor_messages():
    x = fn.factor_input(small())
    with pytest.raises(ValueError, match="'data' must be a dense matrix, dgCMatrix, or path to .spz file"):
        fn.factor_input([1, 2, 3])
    with pytest.raises(ValueError, match=r"Input matrix cannot be empty \(0 rows or 0 columns\)"):
        fn.factor_input(np.zeros((0, 3)))
    with pytest.raises(ValueError, match=r"'input' must be an fn_node \(from factor_input, nmf_layer, etc.\)"):
        fn.nmf_layer(small(), 3)
    with pytest.raises(ValueError, match=r"'W' must be created by W\(\)"):
        fn.nmf_layer(x, 3, W=dict(L1=0.1))
    with pytest.raises(ValueError, match=r"'H' must be created by H\(\)"):
        fn.nmf_layer(x, 3, H=0.1)
    with pytest.raises(ValueError, match="'input' must be an fn_node"):
        fn.svd_layer(None, 3)
    with pytest.raises(ValueError, match="'target' must be a numeric matrix or NULL"):
        fn.H(target=[1.0, 2.0])
    for kind, f in (("shared", fn.factor_shared), ("concat", fn.factor_concat), ("add", fn.factor_add)):
        with pytest.raises(ValueError, match=r"factor_%s\(\) requires at least 2 inputs" % kind):
            f(x)
        with pytest.raises(ValueError, match=r"All arguments to factor_%s\(\) must be fn_node objects" % kind):
            f(x, 3)
    with pytest.raises(ValueError, match=r"factor_add\(\) requires all branches to have the same rank k, got: 4, 3"):
        fn.factor_add(fn.nmf_layer(x, 4), fn.nmf_layer(x, 3))
    with pytest.raises(ValueError, match="'input' must be an fn_node"):
        fn.factor_condition(3, np.ones((2, 2)))
    with pytest.raises(ValueError, match="'Z' must be a numeric matrix"):
        fn.factor_condition(x, "a")
    with pytest.raises(ValueError, match="'inputs' must be fn_node objects"):
        fn.factor_net([x, 3], fn.nmf_layer(x, 2))
    with pytest.raises(ValueError, match="'output' must be an fn_node"):
        fn.factor_net(x, 3)
    with pytest.raises(ValueError, match=r"'config' must be from factor_config\(\)"):
        fn.factor_net(x, fn.nmf_layer(x, 2), config=dict(maxit=3))
    with pytest.raises(ValueError, match="Declared inputs not found in graph: other"):
        fn.factor_net([x, fn.factor_input(small(), "other")], fn.nmf_layer(x, 2))
    with pytest.raises(ValueError, match="'arg' should be one of"):
        fn.factor_config(loss="poisson")
    with pytest.raises(ValueError, match="factor_net has no layers to fit"):
        fn.fit(fn.factor_net(x, x))


def deep(x, cfg=None, **layer_kw):
    return fn.factor_net(x, fn.nmf_layer(fn.nmf_layer(x, 3, **layer_kw), 2), cfg or fn.factor_config())


def test_refusals_name_the_option():
    x = fn.factor_input(small())
    for cfg, word in ((fn.factor_config(loss="gp"), "loss = 'gp'"), (fn.factor_config(test_fraction=0.1), "test_fraction"),
                      (fn.factor_config(precision="fp32"), "precision = 'fp32'")):
        with pytest.raises(NotImplementedError, match=word):
            fn.fit(deep(x, cfg))
    for kw, word in ((dict(L21=0.1), "L21"), (dict(angular=0.1), "angular"), (dict(H=fn.H(graph=np.eye(9), graph_lambda=0.1)), "graph"),
                     (dict(H=fn.H(target=np.ones((3, 9)), target_lambda=0.1)), "target"), (dict(mask="zeros"), "mask"),
                     (dict(zi="row"), "zi"), (dict(projective=True), "projective"), (dict(symmetric=True), "symmetric"),
                     (dict(robust=True), "robust")):
        with pytest.raises(NotImplementedError, match=word):
            fn.fit(deep(x, **kw))
    big = fn.factor_input(small(200, 150))
    with pytest.raises(NotImplementedError, match="a rank above 128"):
        fn.fit(fn.factor_net(big, fn.nmf_layer(fn.nmf_layer(big, 129), 2)))
    y = fn.factor_input(small(7, 9, 2))
    with pytest.raises(NotImplementedError, match=r"Deep NMF with factor_shared\(\) requires single-layer"):
        fn.fit(fn.factor_net([x, y], fn.nmf_layer(fn.nmf_layer(fn.factor_shared(x, y), 3), 2)))
    # single-layer refusals
    for kw, word in ((dict(mask="zeros"), "mask"), (dict(zi="col"), "zi"), (dict(projective=True), "projective"),
                     (dict(symmetric=True), "symmetric"), (dict(robust="mae"), "robust")):
        with pytest.raises(NotImplementedError, match=word):
            fn.fit(fn.factor_net(x, fn.nmf_layer(x, 3, **kw)))
    with pytest.raises(NotImplementedError, match="single svd_layer"):
        fn.fit(fn.factor_net(x, fn.svd_layer(x, 3)))
    with pytest.raises(NotImplementedError, match=".spz path inputs"):
        fn.factor_input(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"))
    res = fn.FactorNetResult({"L1": fn.LayerResult(np.ones((4, 2)), np.ones(2), np.ones((2, 3)), 1, 0.0, False),
                              "L2": fn.LayerResult(np.ones((3, 1)), np.ones(1), np.ones((1, 2)), 1, 0.0, False)}, None, False, None, 1, 0.0, False)
    assert res["L2"] is res.L2 and res.n_layers == 2
    with pytest.raises(NotImplementedError, match="multi-layer"):
        fn.predict(res, np.ones((4, 5)))
    mm = fn.FactorNetResult({"L1": fn.LayerResult({"a": np.ones((4, 2))}, np.ones(2), np.ones((2, 3)), 1, 0.0, False)}, None, True, ["a"], 1, 0.0, False)
    with pytest.raises(ValueError, match="multi-modal results requires matching modality structure"):
        fn.predict(mm, np.ones((4, 5)))


# --------------------------------------------------------------------------------------------------------------- shared stacking
def test_shared_stacking_matches_a_dense_vstack():
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    mats = [rng.uniform(0, 1, (r, 11)) * (rng.uniform(size=(r, 11)) < 0.4) for r in (7, 1, 13)]
    sparse = [fn.factor_input(CSC.from_scipy(sp.csc_matrix(a)), nm) for a, nm in zip(mats, ("a", None, "c"))]
    S, rows = fn.stack_shared(sparse)
    assert isinstance(S, CSC) and rows == [7, 1, 13] and S.shape == (21, 11)
    assert np.array_equal(S.to_scipy().toarray(), np.vstack(mats))
    assert all(np.all(np.diff(S.i[S.p[j]:S.p[j + 1]]) > 0) for j in range(11))          # rows strictly increasing within a column
    mixed = [sparse[0], fn.factor_input(mats[1]), sparse[2]]
    D, rows = fn.stack_shared(mixed)
    assert isinstance(D, np.ndarray) and np.array_equal(D, np.vstack(mats))
    node = fn.factor_shared(*sparse)
    assert node.input_names == ["a", "", "c"]
    with pytest.raises(ValueError, match=r"All inputs to factor_shared\(\) must have the same number of columns"):
        fn.stack_shared([sparse[0], fn.factor_input(np.ones((3, 4)))])


# ------------------------------------------------------------------------------------------------------------------ the symbols
def test_symbols_in_header_and_abi():
    header = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for sym in ("rcppml_hip_graph_assemble", "rcppml_hip_graph_layer_loss", "rcppml_gpu_factor_net_fit_ex"):
        assert sym + "(" in header and sym in _abi.EXPORTED_SYMBOLS
    assert "ops_graph.hip" in open(os.path.join(ROOT, "rcppml_amd", "csrc", "Makefile")).read()
    import rcppml_amd
    assert "factor_net.py" in rcppml_amd.__doc__
