"""CPU checks of the similarity tools: the declarations / exports of the four entries, the numpy specification
(tests/similarity_ref.py) on the known answers of the reference's test_cosine.R and test_bipartiteMatch.R (restated as data), the
library's host assignment solver (rcppml_gpu_bipartite_match_ex, no device) against brute force and scipy, the refusals (nothing
written), the align logic with a planted 3-cycle, and the Python surface's shapes and messages.  No GPU needed."""
import os
import re
import warnings

import numpy as np
import pytest

import similarity_ref as R
from rcppml_amd import _abi
from rcppml_amd import similarity as S
from rcppml_amd.nmf import NMFModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rcppml_gpu_cosine_sparse_ex", "rcppml_gpu_cosine_dense_ex", "rcppml_gpu_bipartite_match_ex")

COST3 = np.array([[1, 0.5, 0.2], [0.5, 1, 0.3], [0.2, 0.3, 1]])                      # test_bipartiteMatch.R:21-23
COST4 = np.array([[10, 8, 1, 9], [7, 10, 6, 2], [3, 5, 8, 7], [6, 4, 9, 8.0]])       # test_bipartiteMatch.R:66-71


def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    for name in NEW:
        m = re.search(r"RCPPML_GPU_API void %s\((.*?)\);" % name, src, flags=re.S)
        assert m, name
        assert [a.strip() for a in m.group(1).split(",")][-1] == "int* out_status"
    assert re.search(r"RCPPML_GPU_API int rcppml_gpu_cosine_geometry\(int64_t\* out\);", src)


def test_library_exports_the_entries():
    L = _abi.lib()
    for name in NEW + ("rcppml_gpu_cosine_geometry",):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(L, name), name


def test_geometry_needs_no_device():
    g = _abi.cosine_geometry()
    assert g["tile"] >= 64 and g["tile"] % 64 == 0 and g["waves"] >= 1
    assert g["tile"] * g["waves"] * 8 <= 160 * 1024            # the tiles of a workgroup fit the CU's LDS
    assert g["groups"] >= 0


def test_package_reexports():
    import rcppml_amd
    assert rcppml_amd.cosine is S.cosine and rcppml_amd.align is S.align and rcppml_amd.bipartiteMatch is S.bipartiteMatch


# ------------------------------------------------------------------------------------------------ the spec on R's known answers
def test_spec_known_matchings():
    for solve in (R.match_ref, R.match_bruteforce):
        a, c = solve(COST3)
        assert c == pytest.approx(1.0) and sorted(a) == [0, 1, 2]
        a, c = solve(COST4)
        assert c == 10 and list(a) == [2, 3, 0, 1]
        a, c = solve(np.eye(3))
        assert c == 0 and all(a[i] != i for i in range(3)) and sorted(a) == [0, 1, 2]      # no fixed point
        a, c = solve(np.zeros((3, 3)))
        assert c == 0 and sorted(a) == [0, 1, 2]
        a, c = solve(np.array([[0.5]]))
        assert c == 0.5 and list(a) == [0]


def test_spec_known_cosines():
    assert R.cosine_ref([1.0, 0, 0], [0, 1.0, 0]) == 0.0
    assert R.cosine_ref([1.0, 0, 0], [1.0, 0, 0]) == 1.0
    g = np.random.default_rng(42)
    A, B, v = g.uniform(size=(5, 6)), g.uniform(size=(5, 4)), g.uniform(size=5)
    C = R.cosine_ref(A)
    assert C.shape == (6, 6) and np.allclose(np.diag(C), 1, atol=1e-10) and np.allclose(C, C.T, atol=1e-10)
    AB = R.cosine_ref(A, B)
    assert AB.shape == (6, 4) and np.all(np.abs(AB) <= 1.01)
    assert R.cosine_ref(A, v).shape == (6,) and R.cosine_ref(v, A).shape == (6,)
    # deviation 1: vector x, matrix y is the cosine (R/cosine.R:47 scales x by |x|^2 instead)
    assert np.allclose(R.cosine_ref(v, A), R.cosine_ref(A, v), atol=1e-15)
    with pytest.raises(ValueError, match="x is a vector and y is NULL"):
        R.cosine_ref(v)


def test_spec_zero_norm_rule_and_sequential_order():
    import scipy.sparse as sp
    g = np.random.default_rng(3)
    A = g.normal(size=(40, 9)) * (g.uniform(size=(40, 9)) < 0.4)
    A[:, 2] = 0
    X = sp.csc_matrix(A)
    C = R.cosine_sparse_ref(X)
    assert np.all(C[2] == 0) and np.all(C[:, 2] == 0)
    seq = R.cosine_sequential(X)
    exact = R.cosine_sequential(X, dtype=np.longdouble)
    nnz = np.diff(X.indptr)
    bound = R.cosine_bound(nnz, nnz)
    assert np.all(seq == seq.T)                                                  # the same chain both ways
    assert np.all(np.abs(seq - exact.astype(np.float64)) <= bound)
    assert np.all(np.abs(C - seq) <= 2 * bound)
    D = R.cosine_dense_ref(A, A)
    assert np.all(np.abs(D - C) <= 2 * R.dense_bound(40))
    K = R.cosine_dense_ref(A[:, :2] + 3.0, A[:, 3:5], "cor")
    assert np.allclose(K, np.corrcoef(A[:, :2].T + 3.0, A[:, 3:5].T)[:2, 2:], atol=1e-12)
    const = np.full((40, 1), 2.0)
    assert np.all(R.cosine_dense_ref(const, A[:, :3], "cor") == 0)               # zero variance


# ------------------------------------------------------------------------------------------------ the host solver through the ABI
def _entry(cost):
    r = _abi.bipartite_match(cost)
    assert r["status"] == 0, r["error"]
    return r["assignment"], r["cost"]


def test_entry_known_answers():
    a, c = _entry(COST4)
    assert list(a) == [2, 3, 0, 1] and c == 10
    a, c = _entry(COST3)
    assert sorted(a) == [0, 1, 2] and c == pytest.approx(1.0)
    a, c = _entry(np.eye(3))
    assert c == 0 and all(a[i] != i for i in range(3))
    assert _entry(np.zeros((3, 3)))[1] == 0
    a, c = _entry(np.array([[0.5]]))
    assert list(a) == [0] and c == 0.5


@pytest.mark.parametrize("nr", range(1, 8))
def test_entry_equals_brute_force(nr):
    g = np.random.default_rng(100 + nr)
    for nc in range(1, 8):
        cost = g.uniform(0.0, 1.0, (nr, nc))                 # continuous: the optimum is unique
        a, c = _entry(cost)
        ba, bc = R.match_bruteforce(cost)
        assert list(a) == list(ba), (nr, nc)
        assert c == pytest.approx(bc, rel=1e-14)
        ra, rc = R.match_ref(cost)
        assert list(ra) == list(a) and rc == pytest.approx(c, rel=1e-14)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 300])
def test_entry_equals_scipy(n):
    opt = pytest.importorskip("scipy.optimize")
    cost = np.random.default_rng(n).uniform(0.0, 1.0, (n, n))
    a, c = _entry(cost)
    rows, cols = opt.linear_sum_assignment(cost)
    assert np.array_equal(a, cols)
    assert c == pytest.approx(cost[rows, cols].sum(), rel=1e-13)
    wide = cost[: max(1, n // 2)]
    a, c = _entry(wide)
    rows, cols = opt.linear_sum_assignment(wide)
    assert np.array_equal(a, cols) and c == pytest.approx(wide[rows, cols].sum(), rel=1e-13)


def test_entry_unmatched_rows_negatives_batch_and_determinism():
    g = np.random.default_rng(5)
    tall = g.uniform(size=(6, 3))
    a, c = _entry(tall)
    assert sorted(a[a >= 0]) == [0, 1, 2] and np.sum(a == -1) == 3
    assert c == pytest.approx(sum(tall[i, a[i]] for i in range(6) if a[i] >= 0))
    neg = np.array([[-5.0, 1.0], [1.0, -2.0]])
    a, c = _entry(neg)
    assert list(a) == [0, 1] and c == 0.0                                        # negatives count as 0
    a2, c2 = _entry(np.array([[0.0, 1.0], [1.0, 0.0]]))
    assert list(a2) == list(a) and c2 == c
    stack = g.uniform(size=(5, 4, 4))
    r = _abi.bipartite_match(stack)
    assert r["status"] == 0 and r["assignment"].shape == (5, 4) and r["cost"].shape == (5,)
    for q in range(5):
        a, c = _entry(stack[q])
        assert np.array_equal(a, r["assignment"][q]) and c == r["cost"][q]
    again = _abi.bipartite_match(stack)
    assert np.array_equal(again["assignment"], r["assignment"]) and np.array_equal(again["cost"], r["cost"])


def test_entry_refusals_leave_outputs_untouched():
    bad = np.ones((3, 3))
    bad[1, 2] = np.nan
    cases = [(_abi.bipartite_match(bad), "non-finite"),
             (_abi.bipartite_match(np.ones((3, 3)) * np.inf), "non-finite"),
             (_abi.bipartite_match(np.ones((2, 2)), nr=0), "nr and nc"),
             (_abi.bipartite_match(np.ones((2, 2)), batch=0), "batch"),
             (_abi.bipartite_match(None, nr=2, nc=2, batch=1), "null cost")]
    for r, word in cases:
        assert r["status"] == -1 and word in r["error"], r["error"]
        asg, tot = r["buffers"]
        assert np.all(asg == -7) and np.all(tot == -7.0)
    st = _abi.C.c_int(-99)
    c = np.ones((2, 2))
    _abi.lib().rcppml_gpu_bipartite_match_ex(_abi._np_ptr(c), _abi._ci(2), _abi._ci(2), _abi._ci(1), None, None, _abi.C.byref(st))
    assert st.value == -1 and "null output" in _abi.last_error()


# ------------------------------------------------------------------------------------------------ align on the spec
def _planted(seed=0, m=50, k=3):
    g = np.random.default_rng(seed)
    w_ref = g.uniform(size=(m, k)) * (g.uniform(size=(m, k)) < 0.5) + 0.01
    sigma = np.array([1, 2, 0])                                                  # object$w[, i] = ref$w[, sigma(i)]: a 3-cycle
    w_obj = w_ref[:, sigma] * g.uniform(0.99, 1.01, size=(m, k))
    return w_ref, w_obj, sigma


def test_align_restores_a_three_cycle():
    w_ref, w_obj, sigma = _planted()
    order, assignment = R.align_ref(w_obj, w_ref)
    assert list(assignment) == list(sigma)                   # assignment[i]: the ref factor matched to object factor i
    aligned = w_obj[:, order]
    sim = R.cosine_dense_ref(aligned, w_ref)
    assert np.all(np.diag(sim) > 0.99)
    off = sim - np.diag(np.diag(sim))
    assert off.max() < 0.9


def test_literal_reading_of_R_stays_misaligned():
    """R/nmf_methods.R:270 indexes the object by the assignment: on a 3-cycle that is sigma applied twice."""
    w_ref, w_obj, sigma = _planted()
    order, _ = R.align_ref(w_obj, w_ref, order_rule=R.align_order_literal_R)
    sim = R.cosine_dense_ref(w_obj[:, order], w_ref)
    assert np.all(np.diag(sim) < 0.9)
    assert list(S.align_order(sigma)) == list(R.align_order(sigma)) != list(R.align_order_literal_R(sigma))
    inv = np.array([1, 0, 2])                                # its own inverse: both readings agree, which is why R's tests pass
    assert list(R.align_order(inv)) == list(R.align_order_literal_R(inv))


def test_similarity_cost_matches_the_spec():
    sim = np.array([[1.0 + 1e-9, 0.3], [-0.2, 1.0]])
    assert np.array_equal(S.similarity_cost(sim), R.similarity_cost(sim))
    assert S.similarity_cost(sim)[0, 0] == 0.0 and S.similarity_cost(sim)[1, 0] == pytest.approx(1.2 + 1e-10)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_surface_messages_and_bipartite_match():
    with pytest.raises(ValueError, match="x is a vector and y is NULL"):
        S.cosine(np.array([1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match="same number of rows"):
        S.cosine(np.ones((3, 2)), np.ones((4, 2)))
    out = S.bipartiteMatch(COST4)
    assert set(out) == {"cost", "assignment"} and out["cost"] == 10 and list(out["assignment"]) == [2, 3, 0, 1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        S.bipartiteMatch(-COST3)                                                 # silent unless verbose
    with pytest.warns(UserWarning, match="Negative values"):
        S.bipartiteMatch(-COST3, verbose=True)
    with pytest.raises(ValueError, match="must be a matrix"):
        S.bipartiteMatch(np.ones(3))


def test_align_checks_before_the_device():
    a = NMFModel(np.ones((5, 2)), np.ones(2), np.ones((2, 4)), {})
    b = NMFModel(np.ones((5, 3)), np.ones(3), np.ones((3, 4)), {})
    with pytest.raises(ValueError, match=r"dimensions of object\$w and ref\$w are not identical"):
        S.align(a, b)
    with pytest.raises(ValueError, match="should be one of"):
        S.align(a, a, method="euclid")
    assert S.align([], a) == []
    mod = NMFModel(np.arange(6.0).reshape(2, 3), np.array([3.0, 2.0, 1.0]), np.arange(12.0).reshape(3, 4), {"tol": 1})
    out = S.permute_model(mod, S.align_order([1, 2, 0]), [1, 2, 0])
    assert np.array_equal(out.w, mod.w[:, [2, 0, 1]]) and np.array_equal(out.d, [1.0, 3.0, 2.0])
    assert np.array_equal(out.h, mod.h[[2, 0, 1]]) and list(out.misc["assignment"]) == [1, 2, 0] and out.misc["tol"] == 1


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_is_loud_and_writes_nothing():
    from rcppml_amd.data import CSC
    X = CSC((3, 2), [0, 1, 2], [0, 2], [1.0, 2.0])
    r = _abi.cosine_sparse(X)
    assert r["status"] == -1 and "no HIP device" in r["error"] and np.all(r["buffers"][0] == -7.0)
    r = _abi.cosine_dense(np.ones((1, 2, 3)), np.ones((2, 3)))
    assert r["status"] == -1 and "no HIP device" in r["error"] and np.all(r["buffers"][0] == -7.0)
    with pytest.raises(_abi.BackendError):
        S.cosine(np.ones((3, 2)))
    assert S.bipartiteMatch(COST3)["cost"] == pytest.approx(1.0)                 # the match needs no device
