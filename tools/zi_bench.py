#!/usr/bin/env python3
"""tools/zi_bench.py -- zero-inflated NB NMF on the GPU path (csrc/ops_zi.hip), one JSON line.
Workload: pbmc3k (tests/golden/pbmc3k.spz, 13 714 genes x 2 700 cells), NB, k = 10, zi = "row", 10 ALS iterations (tol = 0), fp64.
  zi_fit_ms_per_iter     nmf_zi(): wall time of the fit / 10 (set-up, upload and download included)
  nb_fit_ms_per_iter     nmf() with the same arguments and no zero-inflation: the plain sparse NB fit
  zi_stage_ms            rcppml_gpu_zi_em_double alone on the plain fit's model (one E / M round and the imputation, upload and the
                         download of A_imputed included), best of --reps after a warm-up; zi_stage_noimpute_ms: without A_imputed
  zi_ref_stage_ms        the numpy restatement of the stage (tests/zi_ref.py), once (--no-cpu skips it); it is not the reference's time"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, data  # noqa: E402
from rcppml_amd.nmf import nmf  # noqa: E402
from rcppml_amd.zi import nmf_zi  # noqa: E402


def best_of(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))
    k, it = 10, args.iters
    kw = dict(loss="nb", seed=1, maxit=it, tol=0.0, precision="fp64")
    nmf(A, k, **dict(kw, maxit=1))                                  # warm-up: library load, context
    t = time.perf_counter()
    plain = nmf(A, k, **kw)
    nb_s = time.perf_counter() - t
    nmf_zi(A, k, zi="row", **dict(kw, maxit=1))
    t = time.perf_counter()
    mod = nmf_zi(A, k, zi="row", **kw)
    zi_s = time.perf_counter() - t
    W_T, H, d = np.ascontiguousarray(plain.w), np.ascontiguousarray(plain.h.T), plain.d
    disp, pi0 = plain.misc["theta"], np.full(m, 0.2)
    stage = lambda want: _abi.zi_em_double(A, m, n, k, W_T, d, H, disp, pi0, 5, 1, 1, 0.0, want_imputed=want)
    assert stage(True)["status"] == 0
    out = dict(workload="pbmc3k", m=m, n=n, nnz=int(A.nnz), k=k, iters=it, loss="nb", zi="row",
               zi_fit_ms_per_iter=round(zi_s * 1e3 / it, 3), nb_fit_ms_per_iter=round(nb_s * 1e3 / it, 3),
               zi_stage_ms=round(best_of(lambda: stage(True), args.reps) * 1e3, 3),
               zi_stage_noimpute_ms=round(best_of(lambda: stage(False), args.reps) * 1e3, 3),
               zi_loss=mod.misc["loss"], nb_loss=plain.misc["loss"], pi_row_mean=float(np.mean(mod.misc["pi_row"])))
    if not args.no_cpu:
        import zi_ref as Z
        Ao = O.Csc((m, n), A.p, A.i, A.x)
        t = time.perf_counter()
        Z.zi_stage(Ao, W_T, d, H, disp, pi0, Z.NB, Z.ROW, 1)
        out["zi_ref_stage_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
