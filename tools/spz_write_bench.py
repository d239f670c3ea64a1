#!/usr/bin/env python3
"""tools/spz_write_bench.py -- encode time of pbmc3k (13714 x 2700, 2.28 M nonzeros, uint16 counts) on the GPU: the bundled
pbmc3k.spz is decoded (st_read) and written again (rcppml_gpu_spz_write_ex through _abi.spz_write) at the fixture's own chunk
size.  Reports the wall time of the call, its split by stage (HIP events) and the bytes written next to the fixture's, which the
reference encoder wrote.  Prints one JSON line; nothing here is gated in a test."""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcppml_amd import _abi, st_read  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "pbmc3k.spz")
A = st_read(FIXTURE)
chunk_cols = int(np.fromfile(FIXTURE, np.uint32, 32)[6])           # header_v2.hpp:128
with tempfile.TemporaryDirectory() as td:
    path = os.path.join(td, "pbmc3k.spz")
    runs = [_abi._check(_abi.spz_write((A.p, A.i, A.x), A.rows, A.cols, path, -1, chunk_cols, timed=True), "spz_write") for _ in range(8)][3:]
    B = st_read(path)
    assert np.array_equal(A.p, B.p) and np.array_equal(A.i, B.i) and np.array_equal(A.x, B.x)
ms = {k: float(np.median([r["ms"][k] for r in runs])) for k in _abi.SPZ_WRITE_STAGES}
r = runs[0]
print(json.dumps(dict(file="pbmc3k.spz", m=A.rows, n=A.cols, nnz=A.nnz, chunk_cols=chunk_cols, chunks=r["chunks"], value_type=r["value_type"],
                      wall_ms=ms.pop("wall"), stage_ms=ms, symbols_per_s=2 * A.nnz / (ms["encode"] * 1e-3) if ms["encode"] else None,
                      bytes_written=r["bytes"], fixture_bytes=os.path.getsize(FIXTURE),
                      size_ratio_to_fixture=r["bytes"] / os.path.getsize(FIXTURE))))
