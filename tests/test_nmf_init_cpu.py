"""CPU checks of the SVD-seeded NMF start (nmf(seed = "lanczos" | "irlba"), rcppml_gpu_nmf_svd_init_ex): the string seeds and what
nmf() refuses before any device work, the fill rows of the numpy restatement (tests/nmf_init_ref.py) against SplitMix64 written out
by hand, and the two entries in the header and the library.  No compute calls."""
import os
import re

import numpy as np
import pytest

import nmf_init_ref as IR
from rcppml_amd import _abi, nmf as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("rcppml_gpu_nmf_svd_init_ex", "rcppml_gpu_nmf_svd_init_dense_ex")
A = np.abs(np.random.default_rng(5).standard_normal((6, 5)))


def test_seed_strings_map_to_the_reference_init_modes():
    # R/nmf_thin.R:390-403
    assert [N._seed_init_mode(s) for s in ("random", "lanczos", "irlba", "randomized", "svd")] == [0, 1, 2, 1, 1]
    assert N._seed_init_mode(None) is None and N._seed_init_mode(7) is None and N._seed_init_mode(np.ones((6, 2))) is None


@pytest.mark.parametrize("k", [2, [2, 3]])
def test_unknown_seed_string_is_r_s_error(k):
    with pytest.raises(ValueError) as e:
        N.nmf(A, k, seed="lanczoz")
    assert str(e.value) == "Unknown seed string 'lanczoz'. Valid: NULL, integer, matrix, 'lanczos', 'irlba', 'randomized', 'svd'"


@pytest.mark.parametrize("seed", ["lanczos", "irlba", "randomized", "svd"])
def test_h_init_with_an_svd_seed_is_refused(seed):
    with pytest.raises(ValueError) as e:
        N.nmf(A, 2, seed=seed, h_init=np.ones((2, 5)))
    assert str(e.value) == "h_init cannot be combined with an SVD seed: the seed sets both factors"


@pytest.mark.parametrize("bad", [-1, 2 ** 32, 1.5, "7", True, [1, 2]])
def test_svd_seed_is_validated(bad):
    with pytest.raises(ValueError, match="'svd_seed' must be a single integer"):
        N.nmf(A, 2, seed="lanczos", svd_seed=bad)


@pytest.mark.parametrize("seed", [None, 3, "random"])
def test_svd_seed_needs_an_svd_seed_string(seed):
    with pytest.raises(ValueError, match="'svd_seed' needs an SVD seed"):
        N.nmf(A, 2, seed=seed, svd_seed=7)


def splitmix_by_hand(seed, count):
    """rng.hpp:73-74 and :89-96, in Python integers."""
    mask, state, out = (1 << 64) - 1, seed or 12345, []
    for _ in range(count):
        state = (state + 0x9e3779b97f4a7c15) & mask
        z = state
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        out.append(z ^ (z >> 31))
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed, stream", [(0, 54321), (7, 1006), (0xFFFFFFFF, 998), (0xFFFFFFFF - 998, 0)])
def test_fill_rows_by_hand(seed, stream, dtype):
    """2 x 3 input, k = 3 with one triplet delivered: two fill rows a side.  The stream fills the 2 x 2 block of W column by
    column, then goes on into the 2 x 3 block of H; its seed is seed + 999 in uint32 (0xFFFFFFFF wraps to 998), 54321 for 0; a
    sum that wraps to 0 is the generator's 12345."""
    assert IR.fill_seed(seed) == stream
    m, n, k = 2, 3, 3
    U, V, d = np.array([[0.6], [-0.8]]), np.array([[-1.0], [0.0], [0.0]]), np.array([4.0])
    W_T, H = IR.initialize_lanczos(U, d, V, k, m, n, seed, dtype)
    assert W_T.dtype == dtype and H.dtype == dtype and W_T.shape == (m, k) and H.shape == (n, k)
    assert np.array_equal(W_T[:, 0], np.array([1.2, 1.6]).astype(dtype)) and np.array_equal(H[:, 0], [2.0, 0.0, 0.0])
    z = np.array(splitmix_by_hand(stream, 10), np.uint64).astype(dtype) / dtype(2.0 ** 64)      # uniform<T>(), rng.hpp:100-104
    for j in range(m):
        for i in range(2):
            assert W_T[j, 1 + i] == z[j * 2 + i]                 # W_T(1 + i, j): draw j * rows + i
    for j in range(n):
        for i in range(2):
            assert H[j, 1 + i] == z[4 + j * 2 + i]               # H(1 + i, j): the stream goes on after W's 4 draws


def test_no_fill_when_every_triplet_is_delivered():
    rng = np.random.default_rng(0)
    U, V, d = rng.standard_normal((4, 2)), rng.standard_normal((3, 2)), np.array([2.0, 0.5])
    W_T, H = IR.initialize_lanczos(U, d, V, 2, 4, 3, 9)
    assert np.array_equal(W_T, np.abs(U) * np.sqrt(d)) and np.array_equal(H, np.abs(V) * np.sqrt(d))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"RCPPML_GPU_API\s+[\w\s\*]+?\b(rcppml_\w+)\s*\(", src))


def test_header_declares_and_library_exports_both_entries():
    src = open(os.path.join(ROOT, "include", "rcppml_gpu.h")).read()
    declared = _declared_symbols()
    L = _abi.lib()
    for name in ENTRIES:
        assert name in declared and name in _abi.EXPORTED_SYMBOLS and hasattr(L, name)
    # the declaration cites the reference's initialisation it restates
    comment = src[:src.index("RCPPML_GPU_API void rcppml_gpu_nmf_svd_init_ex")].rsplit("/*", 1)[1]
    assert "nmf_init.hpp" in comment


def test_refused_without_touching_the_buffers():
    """k outside [1, min(m, n)] and a bad mode are refused before any device work, on both entries, with the engine's messages."""
    p = np.arange(6, dtype=np.int32) * 6
    i = np.tile(np.arange(6, dtype=np.int32), 5)
    for dense in (False, True):
        for kw, msg in ((dict(k=0), "k_max must be in [1, min(m, n)]"), (dict(k=6), "k_max must be in [1, min(m, n)]"),
                        (dict(k=2, mode=3), "mode must be 1 (lanczos) or 2 (irlba)")):
            bufs = dict(W_T=np.full(6 * 6, 7.0), H=np.full(5 * 6, 7.0), d=np.full(6, 7.0))
            r = _abi.nmf_svd_init(A if dense else (p, i, A.ravel(order="F"), 6, 5), kw["k"], dense=dense, mode=kw.get("mode", 1),
                                  buffers=bufs)
            assert (r["status"], r["error"]) == (-1, msg)
            assert all(np.all(b == 7) for b in bufs.values())
            assert (r["k_svd"], r["iters"], r["wall_ms"]) == (0, 0, 0.0)
