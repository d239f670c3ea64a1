"""GPU tests of the StreamPress v2 writer (rcppml_amd/csrc/ops_spz_write.hip, st_write()): every file is read back bit for bit by
this project's device decoder and by the CPU oracle (oracle/spz_oracle.cpp, pinned to the reference codec: the format check,
which runs none of this project's kernels).  Shapes: the smallest at which each stage can go wrong -- a chunk of one column, empty
columns and chunks, a stream of one encoder block (2048 symbols), one more and several, gaps and values at the escape threshold
and at every varint length, a stream of one symbol, a stream of all 256 with most raw shares below 2^-14, float bit patterns."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
VT = {"uint8": 0, "uint16": 1, "uint32": 2, "fp32": 3, "fp64": 6}
RNG = np.random.default_rng(7)


def _csc(m, cols, vals):
    """CSC of m rows from per-column row arrays; vals: all values in storage order, or a function of their number."""
    from rcppml_amd.data import CSC
    p = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    i = np.concatenate([np.asarray(c, np.int64) for c in cols]) if p[-1] else np.zeros(0, np.int64)
    return CSC((m, len(cols)), p, i, vals(i.size) if callable(vals) else np.asarray(vals, np.float64))


def _random_cols(m, n, empty=()):
    return [np.zeros(0, np.int64) if j in empty else np.sort(RNG.choice(m, RNG.integers(1, m // 2), replace=False)) for j in range(n)]


counts = lambda k: RNG.integers(1, 9, k).astype(np.float64)
normal = lambda k: RNG.standard_normal(k)
LADDER = [254, 255, 256, 65535, 65536, 2 ** 32 - 1]
SPECIAL = [-1.5, -0.0, 5e-324, 1e-40, 1e300, 3.25]
SKEW = np.concatenate([np.arange(256), np.zeros(70000 - 256)])
RNG.shuffle(SKEW)
# name -> (matrix, chunk_cols, [(precision, value type expected)])
CASES = {
    "chunk_of_one_column": (_csc(50, _random_cols(50, 9), counts), 8, [("auto", "uint8"), ("fp64", "fp64"), ("fp32", "fp32")]),
    "float_auto_is_fp64": (_csc(50, _random_cols(50, 9), normal), 8, [("auto", "fp64")]),
    "empty_column_and_chunk": (_csc(40, _random_cols(40, 12, empty=(1, 4, 5, 6, 7)), counts), 4, [("auto", "uint8"), ("fp64", "fp64")]),
    "one_block": (_csc(6000, [np.arange(2048)], lambda k: RNG.integers(0, 300, k)), 2048, [("auto", "uint16")]),
    "one_block_plus_1": (_csc(6000, [np.arange(2049) * 2], lambda k: RNG.integers(0, 300, k)), 2048, [("auto", "uint16"), ("fp64", "fp64")]),
    "several_blocks": (_csc(6000, [np.arange(5000)], lambda k: RNG.integers(0, 300, k)), 2048, [("auto", "uint16"), ("fp32", "fp32")]),
    "gap_ladder": (_csc(70000, [np.cumsum(np.array([0, 254, 255, 256, 16383, 16384]) + 1) - 1], counts), 2048, [("auto", "uint8")]),
    "value_ladder": (_csc(10, [np.arange(6)], LADDER), 2048, [("auto", "uint32"), ("uint32", "uint32"), ("fp64", "fp64")]),
    "value_ladder_u16": (_csc(10, [np.arange(4)], LADDER[:4]), 2048, [("auto", "uint16"), ("uint16", "uint16"), ("uint32", "uint32")]),
    "value_ladder_u8": (_csc(10, [np.arange(2)], LADDER[:2]), 2048, [("auto", "uint8"), ("uint8", "uint8"), ("uint16", "uint16")]),
    "single_symbol": (_csc(300, [np.arange(300)], np.ones(300)), 2048, [("auto", "uint8"), ("fp64", "fp64")]),
    "all_symbols_skewed": (_csc(70000, [np.arange(70000)], SKEW), 2048, [("auto", "uint8")]),
    "float_bit_patterns": (_csc(6, [np.arange(6)], SPECIAL), 2048, [("auto", "fp64"), ("fp64", "fp64"), ("fp32", "fp32")]),
    "no_nonzeros": (_csc(5, [[], []], []), 2048, [("auto", "uint8"), ("fp64", "fp64")]),
}


@pytest.fixture(scope="module")
def env():
    import torch
    from rcppml_amd import _abi
    return torch, _abi, _abi.Context(0)


@pytest.mark.parametrize("name,precision,expect", [(k, p, e) for k, (_, _, kinds) in CASES.items() for p, e in kinds])
def test_round_trip_is_bit_exact(env, tmp_path, name, precision, expect):
    import rcppml_amd
    torch, _abi, ctx = env
    A, chunk_cols, _ = CASES[name]
    path = tmp_path / "a.spz"
    r = rcppml_amd.st_write(A, path, precision=precision, chunk_cols=chunk_cols)
    buf = np.fromfile(path, np.uint8)
    assert r == dict(bytes=buf.size, value_type=expect, chunks=-(-A.cols // chunk_cols), nnz=A.nnz)
    assert _abi.spz_info(buf) == (0, A.rows, A.cols, A.nnz, VT[expect])
    with np.errstate(over="ignore"):
        x = A.x.astype(np.float32).astype(np.float64) if precision == "fp32" else A.x
    dp = torch.full((A.cols + 1,), -7, dtype=torch.int32, device="cuda")
    di = torch.full((max(A.nnz, 1),), -7, dtype=torch.int32, device="cuda")
    dx = torch.full((max(A.nnz, 1),), -7.0, dtype=torch.float64, device="cuda")
    ctx.spz_decode(buf, dp, di, dx)
    for p, i, v in ((dp.cpu().numpy(), di.cpu().numpy()[:A.nnz], dx.cpu().numpy()[:A.nnz]), O.spz_decode(buf)):
        assert np.array_equal(p.astype(np.int64), A.p) and np.array_equal(i.astype(np.int64), A.i)
        assert np.array_equal(v.view(np.uint64), x.view(np.uint64))
    B = rcppml_amd.st_read(path)
    assert B.shape == A.shape and np.array_equal(B.i, A.i) and np.array_equal(B.x.view(np.uint64), x.view(np.uint64))
    assert rcppml_amd.st_info(path) == dict(m=A.rows, n=A.cols, nnz=A.nnz, value_type=expect, bytes=buf.size)


def test_refusals_leave_no_file(env, tmp_path):
    import rcppml_amd
    _, _abi, _ = env
    path = tmp_path / "no.spz"
    A = _csc(10, [np.arange(4)], [1, 2, 3, 4])
    A.i[:] = [0, 2, 2, 3]                                            # rows do not ascend
    with pytest.raises(_abi.BackendError, match="strictly increasing"):
        rcppml_amd.st_write(A, path)
    A.i[:] = [0, 1, 2, 10]                                           # a row outside the matrix
    with pytest.raises(_abi.BackendError, match="strictly increasing"):
        rcppml_amd.st_write(A, path)
    for vals, precision in (([1, 2.5, 3, 4], "uint8"), ([1, 2, 3, 256], "uint8"), ([1, 2, 3, 65536], "uint16"), ([1, 2, -3, 4], "uint32"),
                            ([1, 2, 3, 2.0 ** 32], "uint32")):
        with pytest.raises(ValueError, match="fits"):
            rcppml_amd.st_write(_csc(10, [np.arange(4)], vals), path, precision=precision)
    good = _csc(10, [np.arange(4)], [1, 2, 3, 4])
    with pytest.raises(NotImplementedError, match="fp16"):
        rcppml_amd.st_write(good, path, precision="fp16")
    with pytest.raises(NotImplementedError, match="row_sort"):
        rcppml_amd.st_write(good, path, row_sort=True)
    with pytest.raises(ValueError, match="chunk_cols"):
        rcppml_amd.st_write(good, path, chunk_cols=0)
    assert not path.exists()


@pytest.mark.parametrize("name,precision", [("empty_column_and_chunk", "auto"), ("several_blocks", "fp32"), ("all_symbols_skewed", "auto")])
def test_two_writes_are_identical(tmp_path, name, precision):
    import rcppml_amd
    A, chunk_cols, _ = CASES[name]
    for f in ("a.spz", "b.spz"):
        rcppml_amd.st_write(A, tmp_path / f, precision=precision, chunk_cols=chunk_cols)
    assert (tmp_path / "a.spz").read_bytes() == (tmp_path / "b.spz").read_bytes()


def test_streamed_fits_take_the_written_file(tmp_path):
    """README: the streamed fits give the same bits from an .spz file as from the CSC at equal panel boundaries."""
    import rcppml_amd
    A = _csc(40, _random_cols(40, 24), normal)
    A.x[:] = np.abs(A.x)
    path = tmp_path / "fit.spz"
    rcppml_amd.st_write(A, path, chunk_cols=8)
    a = rcppml_amd.nmf_streaming(str(path), k=4, maxit=3, seed=1, precision="fp64", panel_cols=8)
    b = rcppml_amd.nmf_streaming(A, k=4, maxit=3, seed=1, precision="fp64", panel_cols=8)
    assert np.array_equal(a.w, b.w) and np.array_equal(a.d, b.d) and np.array_equal(a.h, b.h)
    a = rcppml_amd.svd_streaming(str(path), k=3, seed=1, precision="double", panel_cols=8)
    b = rcppml_amd.svd_streaming(A, k=3, seed=1, precision="double", panel_cols=8)
    assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["d"], b["d"]) and np.array_equal(a["v"], b["v"])
