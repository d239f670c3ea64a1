"""What tests/svd_geometry_inputs.py promises tests/test_gpu_svd_geometry.py, proved without a device: the shapes cross the SVD
kernels' chunk the way their table says, every factored matrix has a spaced spectrum, the float64 restatement is within 1e-11 of
its longdouble run, the fixed iteration counts hold in both precisions, every CV case holds out more than two chunks, and MEASURED
is what the restatement gives.  No GPU needed."""
import functools
import os
import re

import numpy as np
import pytest

import svd_cv_ref as C
import svd_geometry_inputs as G
import svd_ref as P
import svd_reg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "rcppml_amd", "csrc", "kernels_svd.hip.h")
IDS = dict(ids=G.case_id)


def header_constants():
    """WG and PER from their two constexpr lines."""
    src = open(HEADER).read()
    wg = re.search(r"^constexpr int WG = (\d+),", src, flags=re.M)
    per = re.search(r"^constexpr int PER = (\d+), CH = WG \* PER;", src, flags=re.M)
    assert wg and per, "kernels_svd.hip.h no longer declares WG and PER the way this test reads them"
    return int(wg.group(1)), int(per.group(1))


# ------------------------------------------------------------------------------------------------ shapes
def test_shape_table_still_crosses_the_chunk_as_it_says():
    wg, per = header_constants()
    ch = wg * per
    assert (ch, wg) == (G.CHUNK, G.TILE)
    nb = {name: (G.nblk(s["m"], ch), G.nblk(s["n"], ch)) for name, s in G.ALL_SHAPES.items()}
    assert nb == {"2048x2049": (1, 2), "4097x63": (3, 1), "63x6145": (1, 4), "2051x4099": (2, 3), "1x2049": (1, 2), "2049x1": (2, 1)}
    lens = [s[key] for s in G.ALL_SHAPES.values() for key in ("m", "n")]
    assert any(l % ch == 0 for l in lens)                                    # a chunk that is exactly full, no tail
    assert sum(l > ch and l % ch == 1 for l in lens) >= 4                    # a last chunk of one element
    assert any(a != b and a > 1 and b > 1 for a, b in nb.values())           # nbm != nbn, both above one
    assert G.SHAPES["4097x63"]["n"] < 64 and G.SHAPES["63x6145"]["m"] < 64  # below one wavefront
    # nmf_start_kernel tiles rows by WG: the lengths straddle it, three blocks and two, each with one row in the last
    tiles = sorted({(-(-l // wg), l % wg) for mn in G.NMF_SHAPES.values() for l in mn})
    assert tiles == [(2, 1), (3, 1)] and G.NMF_RANKS == (5, 33)


def test_case_tables_cover_what_they_list():
    assert len(set(G.PARITY_CASES)) == len(G.PARITY_CASES) == 40 + 8 + 8
    for s in G.ALL_SHAPES:
        for kd in G.KINDS:
            assert any(c[1] == s and c[2] == kd for c in G.DEFLATION_CASES) and any(c[:2] == (s, kd) for c in G.LANCZOS_CASES)
    assert {c[1] for c in G.REG_CASES} == {"2051x4099", "4097x63"} and {c[1] for c in G.CV_CASES} == {"2051x4099", "63x6145"}
    assert all(c in G.PARITY_CASES and G.case_kind(c) == "csc" and c[1] == "2051x4099" for c in G.DETERMINISM_CASES)
    assert {c[0] for c in G.DETERMINISM_CASES} == {"defl", "reg", "cv"}
    assert [G.lanczos_k(s) for s in G.ALL_SHAPES] == [5, 5, 5, 5, 1, 1]
    assert all(not c[3] and G.case_k(c) == 1 for c in G.DEFLATION_CASES if c[1] in G.DEGENERATE)
    for c in G.REG_CASES:                                                    # every term on at once, the graphs clear of the amplifying range
        kw = G.case_kwargs(c)[2]
        assert min(kw["L21"]) > 0 and min(kw["angular"]) > 0 and min(kw["graph_lambda"]) > 0
        assert (kw["graph_u"][3], kw["graph_v"][3]) == (G.ALL_SHAPES[c[1]]["m"], G.ALL_SHAPES[c[1]]["n"])
        assert all(l * R.lambda_max_bound(g) <= 0.4 for l, g in zip(kw["graph_lambda"], (kw["graph_u"], kw["graph_v"])))
    masked = [c for c in G.CV_CASES if G.case_kwargs(c)[2].get("obs_mask") is not None]
    assert masked and all(G.case_kind(c) == "csc" and abs(G.case_kwargs(c)[2]["obs_mask"].mean() - 0.05) < 0.002 for c in masked)
    assert all(G.case_kwargs(c)[2]["tol"] == 0.0 for c in G.PARITY_CASES)


def test_sparse_patterns():
    A, keep = G.shape_input("2051x4099", "csc")
    assert not keep[G.EMPTY_ROW].any() and not keep[:, G.EMPTY_COL].any()
    assert keep.any(axis=1).sum() == 2050 and keep.any(axis=0).sum() == 4098
    for s, spec in G.ALL_SHAPES.items():
        A, keep = G.shape_input(s, "csc")
        assert A.shape == (spec["m"], spec["n"]) and np.all(A[~keep] == 0) and abs(keep.mean() - spec["density"]) < 0.02
        assert G.shape_input(s, "dense")[1] is None
        assert np.array_equal(G.shape_input(s, "csc", True)[1], keep)            # the level changes values, not the pattern


# ------------------------------------------------------------------------------------------------ spectrum
@functools.lru_cache(maxsize=None)
def leading_values(shape, kind, center, masked, held_out):
    """The leading singular values of the matrix a case factors; cases that factor the same matrix share one decomposition."""
    case = next(c for c in G.PARITY_CASES if matrix_key(c) == (shape, kind, center, masked, held_out))
    return np.linalg.svd(G.factored_matrix(case), compute_uv=False)[:G.case_k(case) + 1]


def matrix_key(case):
    kw = G.case_kwargs(case)[2]
    return (case[1], G.case_kind(case), bool(kw.get("center")), kw.get("obs_mask") is not None, kw.get("test_fraction", 0) > 0)


@pytest.mark.parametrize("case", [c for c in G.PARITY_CASES if c[1] not in G.DEGENERATE], **IDS)
def test_leading_singular_values_are_spaced_by_at_most_08(case):
    """A condition on the inputs, not a tolerance.  The Lanczos inputs are the matrices of the plain deflation cases."""
    sv = leading_values(*matrix_key(case))
    assert sv.size == G.case_k(case) + 1 and np.all(sv[1:] / sv[:-1] <= 0.8), sv[1:] / sv[:-1]


def test_degenerate_inputs_have_one_singular_value():
    for c in G.DEFLATION_CASES:
        if c[1] in G.DEGENERATE:
            assert min(G.factored_matrix(c).shape) == 1 and np.linalg.norm(G.factored_matrix(c)) > 1


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("case", G.PARITY_CASES, **IDS)
def test_float64_restatement_is_within_1e11_of_longdouble(case):
    a, b = G.case_ref(case, np.float64), G.case_ref(case, np.longdouble)
    assert np.array_equal(a["iters"], b["iters"]) and (a["k_selected"], a["k_computed"]) == (b["k_selected"], b["k_computed"])
    assert R.deviation(a, b) < 1e-11
    if a["test_loss"].size:
        tl = b["test_loss"].astype(np.float64)
        assert np.all(np.abs(a["test_loss"] - tl) < 1e-11 * tl)


@pytest.mark.parametrize("case", G.PARITY_CASES, **IDS)
def test_fixed_iteration_counts_hold_in_both_precisions(case):
    """tol = 0 ends a factor only on a rounded-negative distance; 100 eps of room keeps the count the same in the restatement and
    on the device.  A degenerate shape runs one iteration, which counts one converged or not."""
    for dt in (np.float32, np.float64):
        r = G.case_ref(case, dt)
        assert r["k_selected"] == r["k_computed"] == G.case_k(case) and np.all(r["iters"] == G.case_iters(case))
        assert np.all(r["d"] > 0)
        if case[1] in G.DEGENERATE:
            assert G.case_iters(case) == 1
            continue
        for d in r["dist"]:
            assert len(d) == G.case_iters(case) and min(d) > 100 * np.finfo(dt).eps, (dt, min(d))


def test_with_the_terms_off_the_reference_is_the_plain_and_the_cv_restatement_bitwise():
    case = ("defl", "4097x63", "csc", True, "l1nn")
    A, keep, kw = G.case_kwargs(case)
    a, b = G.case_ref(case), P.deflation_svd(A, G.case_k(case), **kw)
    for key in ("u", "d", "v", "iters", "row_means"):
        assert np.array_equal(a[key], b[key]), key
    assert a["frob"] == b["frob"]
    case = ("cv", "63x6145", "csc_obs_mask_center")
    A, keep, kw = G.case_kwargs(case)
    a, b = G.case_ref(case), C.cv_deflation_svd(A, G.case_k(case), stored=keep, **kw)
    for key in ("u", "d", "v", "iters", "test_loss", "rows", "cols"):
        assert np.array_equal(a[key], b[key]), key
    assert (a["n_test"], a["n_masked"], a["frob"]) == (b["n_test"], b["n_masked"], b["frob"])


@pytest.mark.parametrize("case", G.CV_CASES, **IDS)
def test_cv_cases_hold_out_more_than_two_chunks(case):
    r = G.case_ref(case)
    wg, per = header_constants()
    assert r["n_test"] > 2 * wg * per and r["test_loss"].size == G.case_k(case) and np.all(r["test_loss"] > 0)
    if G.case_kwargs(case)[2].get("obs_mask") is not None:
        assert r["n_masked"] > 0


# ------------------------------------------------------------------------------------------------ MEASURED
def test_measured_has_every_case():
    assert set(G.MEASURED) == set(G.PARITY_CASES)


@pytest.mark.parametrize("case", G.PARITY_CASES, **IDS)
def test_measured_is_the_restatements_own_float32_deviation(case):
    dev = G.measured(case)
    assert G.MEASURED[case] / 1.05 <= dev <= G.MEASURED[case] * 1.05, (dev, G.MEASURED[case])
