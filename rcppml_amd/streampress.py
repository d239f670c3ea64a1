"""st_write() / st_read() / st_info(): the reference's StreamPress file surface (R/streampress.R:69, :145, :166) for v2 `.spz`
files, on the HIP codec paths -- the writer of csrc/ops_spz_write.hip and the reader of csrc/ops_spz.hip.  Both run the entropy
coding on the device; neither has a host fallback.

st_write() produces what nmf_streaming(), svd_streaming() and sp_read_gpu take: a v2 file, not row-sorted, without a transpose
section.  It writes the lossless value types only, so st_read(st_write(x)) returns x bit for bit ("fp32" excepted, which rounds
the values to fp32 first).  The bytes are not the reference encoder's -- the frequency tables are normalised by a rule of this
build (csrc/kernels_spz_write.hip.h) -- but every v2 decoder reads them: a stream carries its own table.
"""
import os

import numpy as np

from . import _abi
from .data import CSC
from .nmf import _as_csc

DEFAULT_CHUNK_COLS = 2048                     # header_v2.hpp:39
_NAMES = {0: "uint8", 1: "uint16", 2: "uint32", 3: "fp32", 4: "fp16", 5: "quant8", 6: "fp64"}
# what this writer does not produce, by argument: refused before anything runs
_REFUSED = dict(row_sort=False, include_transpose=False, obs=None, var=None, version=2)


def st_write(x, path, precision="auto", chunk_cols=DEFAULT_CHUNK_COLS, **unsupported):
    """Write `x` (a scipy sparse matrix, a CSC, or a 2-D array taken as sparse) to `path` as a StreamPress v2 file.

    precision: "auto" stores non-negative integer data below 2^32 in the smallest of uint8 / uint16 / uint32 and anything else as
    fp64 byte planes, both lossless; "fp64" and "fp32" force byte-shuffled float planes ("fp32" rounds); "uint8" | "uint16" |
    "uint32" force an integer type and raise ValueError when a stored value is not a non-negative integer that fits it.  "fp16" and
    "quant8" are lossy and raise NotImplementedError, as do row_sort, include_transpose, obs, var and version set to anything but
    their defaults.  chunk_cols: columns per chunk, 1 .. 2^31 - 1; the streamed fits take panels of whole chunks.
    Returns dict(bytes, value_type, chunks, nnz).  Nothing is written when the call fails."""
    for name, value in unsupported.items():
        if name not in _REFUSED:
            raise TypeError("st_write() got an unexpected keyword argument '%s'" % name)
        default = _REFUSED[name]
        if not (value is None if default is None else (np.ndim(value) == 0 and value == default)):
            raise NotImplementedError("st_write(): '%s' is not produced by this writer" % name)
    if precision in ("fp16", "quant8"):
        raise NotImplementedError("st_write(): precision '%s' is lossy and is not produced by this writer" % precision)
    if precision != "auto" and precision not in _abi.SPZ_VALUE_TYPES:
        raise ValueError("precision must be 'auto', 'fp32', 'fp64', 'uint8', 'uint16' or 'uint32'")
    if not 1 <= int(chunk_cols) <= 2 ** 31 - 1:
        raise ValueError("'chunk_cols' must be in [1, 2^31 - 1]")
    A = _as_csc(x)
    path = os.fspath(path)
    r = _abi.spz_write((A.p, A.i, A.x), A.rows, A.cols, path, _abi.SPZ_VALUE_TYPES.get(precision, -1), int(chunk_cols))
    if r["status"] == 2:
        raise ValueError("st_write(): %s" % r["error"])
    _abi._check(r, "spz_write")
    return dict(bytes=r["bytes"], value_type=_NAMES[r["value_type"]], chunks=r["chunks"], nnz=r["nnz"])


def st_info(path):
    """Header of a v2 .spz file: dict(m, n, nnz, value_type, bytes).  Host only."""
    path = os.fspath(path)
    st, m, n, nnz, vt = _abi.spz_info(np.fromfile(path, np.uint8, 128))
    if st != 0:
        raise ValueError("%s is not a v2 .spz file" % (path,))
    return dict(m=m, n=n, nnz=nnz, value_type=_NAMES.get(vt, "unknown"), bytes=os.path.getsize(path))


def st_read(path, device=0):
    """Decode a v2 .spz file on the device (csrc/ops_spz.hip) and return it as a host CSC."""
    import torch
    buf = np.fromfile(os.fspath(path), np.uint8)
    st, m, n, nnz, _ = _abi.spz_info(buf)
    if st != 0:
        raise ValueError("%s is not a v2 .spz file" % (path,))
    ctx = _abi.Context(device)
    try:
        dev = "cuda:%d" % device
        dp = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        di = torch.zeros(max(nnz, 1), dtype=torch.int32, device=dev)
        dx = torch.zeros(max(nnz, 1), dtype=torch.float64, device=dev)
        ctx.spz_decode(buf, dp, di, dx)
        return CSC((m, n), dp.cpu().numpy(), di.cpu().numpy()[:nnz], dx.cpu().numpy()[:nnz])
    finally:
        ctx.close()
