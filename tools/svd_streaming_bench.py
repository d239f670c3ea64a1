"""Panel-streamed randomized PCA against the resident one on pbmc3k (tests/golden/pbmc3k.spz, genes x cells, pca(k = 40), l = 50), both
precisions: wall time of svd(method = "randomized") and of svd_streaming() from the host CSC at 256 / 1024 / all columns per panel
and from the .spz file itself, the bytes of the panel buffer against the resident CSC + CSR, and per pass over the panels the time
of rcppml_hip_stream_block_prod against rs_prod_kernel on the resident CSR (read off the resident fit: its 2 q + 2 products are
all but its whole time, so the figure is an upper bound) and against rcppml_hip_stream_rhs_w at l = 32 and 64.  Prints one JSON line.

    python tools/svd_streaming_bench.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return 1e3 * min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from rcppml_amd import _abi, pca_streaming
    from rcppml_amd.svd import pca
    from streaming_bench import read_spz
    spz = os.path.join(ROOT, "tests", "golden", "pbmc3k.spz")
    A = read_spz(spz)
    m, n, k, l = A.rows, A.cols, 40, 50
    res = dict(tool="svd_streaming_bench", workload="pbmc3k", m=m, n=n, nnz=A.nnz, k=k, sketch=l, power_iterations=3,
               resident_bytes=2 * (12 * A.nnz) + 4 * (m + n + 2), precisions=[])
    ctx = _abi.Context(0)
    dev = lambda v, t=None: torch.from_numpy(np.ascontiguousarray(v)).to("cuda", t)

    def timed(fn):
        fn()
        ctx.sync()
        return best(lambda: (fn(), ctx.sync()), a.reps)

    for precision, dt, td in (("float", _abi.F32, torch.float32), ("double", _abi.F64, torch.float64)):
        kw = dict(seed=7, precision=precision)
        pca(A, k, method="randomized", **kw)                     # first-use costs stay out of the timings
        row = dict(precision=precision, resident_ms=best(lambda: pca(A, k, method="randomized", **kw), a.reps), panels=[])
        row["resident_ms_per_product_upper_bound"] = row["resident_ms"] / 8
        for pc in (256, 1024, n):
            st = pca_streaming(A, k, panel_cols=pc, **kw)
            parts = [A.col_slice(j, min(j + pc, n)) for j in range(0, n, pc)]
            parts = [(dev(c.p), dev(np.append(c.i, 0).astype(np.int32)), dev(np.append(c.x, 0.0), td), c.cols) for c in parts]
            entry = dict(panel_cols=pc, **{key: st["misc"][key] for key in ("panels", "passes", "panel_bytes_peak", "range_table_bytes", "device_ops")})
            entry["panel_bytes_over_resident"] = st["misc"]["panel_bytes_peak"] / res["resident_bytes"]
            entry["streaming_ms"] = best(lambda: pca_streaming(A, k, panel_cols=pc, **kw), a.reps)
            entry["streaming_spz_ms"] = best(lambda: pca_streaming(spz, k, panel_cols=pc, **kw), max(a.reps // 2, 1))
            for width in (32, l, 64, 128):
                X = torch.rand((n, width), dtype=td, device="cuda")
                Y = torch.empty((m, width), dtype=td, device="cuda")

                def scatter_pass():
                    j = 0
                    for q, (p, i, x, cols) in enumerate(parts):
                        _abi.stream_block_prod(ctx, dt, p, i, x, m, cols, width, X[j:j + cols], q > 0, Y)
                        j += cols

                def rhs_w_pass():
                    j = 0
                    for q, (p, i, x, cols) in enumerate(parts):
                        ctx.stream_rhs_w(dt, p, i, x, cols, m, X[j:j + cols], width, q > 0, Y)
                        j += cols

                entry["scatter_ms_per_pass_l%d" % width] = timed(scatter_pass)
                if width in (32, 64):
                    entry["stream_rhs_w_ms_per_pass_k%d" % width] = timed(rhs_w_pass)
            row["panels"].append(entry)
        res["precisions"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
