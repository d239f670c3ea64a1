"""Panel-streamed NMF against the resident fit on pbmc3k (tests/golden/pbmc3k.spz, genes x cells, k = 32): wall time per iteration
of nmf_streaming() at several panel widths (from the host CSC and from the .spz file itself) and of nmf(), the bytes of the panel
buffer against the resident CSC + transpose, and
the time of rcppml_hip_stream_rhs_w per pass over the panels against rcppml_hip_rhs on the resident transpose (pbmc3k is below the
size at which the resident fit plans its right-hand sides).  Prints one JSON line.

    python tools/streaming_bench.py [--iters 10] [--reps 3] [--precision fp32]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_spz(path):
    """The matrix of an .spz file as a host CSC, through the device decoder."""
    import torch
    from rcppml_amd import _abi
    from rcppml_amd.data import CSC
    raw = np.fromfile(path, np.uint8)
    st, m, n, nnz, _ = _abi.spz_info(raw)
    assert st == 0
    ctx = _abi.Context(0)
    p = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    i = torch.empty(nnz, dtype=torch.int32, device="cuda")
    x = torch.empty(nnz, dtype=torch.float64, device="cuda")
    ctx.spz_decode(raw, p, i, x)
    ctx.sync()
    return CSC((m, n), p.cpu().numpy(), i.cpu().numpy(), x.cpu().numpy())


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    a = ap.parse_args()
    import torch
    from rcppml_amd import _abi, nmf_streaming
    from rcppml_amd.nmf import nmf
    A = read_spz(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"))
    m, n, k = A.rows, A.cols, 32
    kw = dict(tol=0.0, maxit=a.iters, seed=7, precision=a.precision, solver="cd")
    nmf(A, k, **kw)                                              # first-use costs (library load, kernel upload) stay out of the timings
    res = dict(tool="streaming_bench", workload="pbmc3k", m=m, n=n, nnz=A.nnz, k=k, precision=a.precision, iters=a.iters,
               resident_bytes=2 * (12 * A.nnz) + 4 * (m + n + 2),
               nmf_ms_per_iter=1e3 * best(lambda: nmf(A, k, **kw), a.reps) / a.iters, panels=[])
    dt, td = (_abi.F32, torch.float32) if a.precision == "fp32" else (_abi.F64, torch.float64)
    ctx = _abi.Context(0)
    dev = lambda v, t=None: torch.from_numpy(np.ascontiguousarray(v)).to("cuda", t)
    H = torch.rand((n, k), dtype=td, device="cuda")
    B = torch.empty((m, k), dtype=td, device="cuda")
    At = A.transpose()
    tp, ti, tx = dev(At.p), dev(At.i), dev(At.x, td)

    def timed(fn):
        fn()
        ctx.sync()
        return 1e3 * best(lambda: (fn(), ctx.sync()), a.reps)

    res["rhs_resident_transpose_ms"] = timed(lambda: ctx.rhs(dt, tp, ti, tx, m, H, k, B))
    for pc in (256, 512, 1024, n):
        st = nmf_streaming(A, k, panel_cols=pc, **kw)
        slices = [(j, min(j + pc, n)) for j in range(0, n, pc)]
        parts = [(A.col_slice(j0, j1), H[j0:j1]) for j0, j1 in slices]
        parts = [((dev(c.p), dev(np.append(c.i, 0).astype(np.int32)), dev(np.append(c.x, 0.0), td)), c.cols, h) for c, h in parts]

        def one_pass():
            for q, ((p, i, x), cols, h) in enumerate(parts):
                ctx.stream_rhs_w(dt, p, i, x, cols, m, h, k, q > 0, B)

        spz = os.path.join(ROOT, "tests", "golden", "pbmc3k.spz")
        res["panels"].append(dict(panel_cols=pc, panels=st.misc["panels"], panel_bytes_peak=st.misc["panel_bytes_peak"],
                                  range_table_bytes=st.misc["range_table_bytes"], device_ops_per_iter=st.misc["device_ops_per_iter"],
                                  panel_bytes_over_resident=st.misc["panel_bytes_peak"] / res["resident_bytes"],
                                  streaming_ms_per_iter=1e3 * best(lambda: nmf_streaming(A, k, panel_cols=pc, **kw), a.reps) / a.iters,
                                  streaming_spz_ms_per_iter=1e3 * best(lambda: nmf_streaming(spz, k, panel_cols=pc, **kw), a.reps) / a.iters,
                                  loss=st.misc["loss"], stream_rhs_w_ms_per_pass=timed(one_pass)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
