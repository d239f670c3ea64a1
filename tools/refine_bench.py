#!/usr/bin/env python3
"""tools/refine_bench.py -- label-guided refinement on the GPU path (csrc/ops_refine.hip).
Workload: pbmc3k (tests/golden/pbmc3k.spz: 13 714 genes x 2 700 cells), k = 10; the labels are the argmax over the factors of an
independent fit's H (another seed).  Printed as one JSON line, each the median of --repeat (default 5) runs after one warm-up:
compute_target (the entry end to end: upload of H, kernels, host k x C stage, download of the target), one refine cycle (the entry
end to end with cycles = 1 minus the same call with cycles = 0, and both raw figures), and the numpy restatement
(tests/refine_ref.py, on a scipy CSC) of the same two on the same inputs (the CPU reference of the tests, not R's time)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, nmf as nmf_module  # noqa: E402
from rcppml_amd.data import CSC  # noqa: E402


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    return sp.csc_matrix((np.asarray(x, np.float64), np.asarray(i), np.asarray(p)), shape=(m, n))


def median_of(fn, repeat):
    r = fn()                                             # warm-up
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ref-repeat", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.8)
    args = ap.parse_args()
    if not _abi.detect():
        raise SystemExit("refine_bench needs a GPU")
    import refine_ref as R
    S = pbmc3k()
    A = CSC.from_scipy(S)
    m, n = S.shape
    k = args.k
    model = nmf_module.nmf(A, k, seed=args.seed, precision="fp64")
    other = nmf_module.nmf(A, k, seed=args.seed + 1, precision="fp64")
    codes = np.argmax(other.h, axis=0).astype(np.int32)
    C = int(codes.max()) + 1
    H = np.ascontiguousarray(model.h.T)

    r, t_target = median_of(lambda: _abi.compute_target_double(H, codes, C, True), args.repeat)
    assert r["status"] == 0, r["error"]

    def dev(cycles):
        return _abi.refine_double(A, None, m, n, k, model.w, model.d, H, codes, C, args.lam, cycles, True, True)

    r0, t0 = median_of(lambda: dev(0), args.repeat)
    r1, t1 = median_of(lambda: dev(1), args.repeat)
    assert r0["status"] == 0 and r1["status"] == 0, (r0["error"], r1["error"])
    ref_t, tr_target = median_of(lambda: R.compute_target(model.h, codes, C, True), args.ref_repeat)
    ref0, tr0 = median_of(lambda: R.refine(model.w, model.d, model.h, S, codes, C, args.lam, 0), args.ref_repeat)
    ref1, tr1 = median_of(lambda: R.refine(model.w, model.d, model.h, S, codes, C, args.lam, 1), args.ref_repeat)
    print(json.dumps(dict(workload="pbmc3k", m=m, n=n, nnz=int(S.nnz), k=k, classes=C, class_sizes=np.bincount(codes, minlength=C).tolist(),
                          compute_target_device_s=t_target, refine_cycles0_device_s=t0, refine_cycles1_device_s=t1,
                          refine_one_cycle_device_s=t1 - t0, restatement_compute_target_s=tr_target, restatement_refine_cycles0_s=tr0,
                          restatement_refine_cycles1_s=tr1, restatement_one_cycle_s=tr1 - tr0,
                          restatement_label="numpy restatement (tests/refine_ref.py), not the reference's code",
                          target_rel_diff=R.rel_diff(r["target"].T, ref_t), cycle1_H_corr_rel_diff=R.rel_diff(r1["H_corr"].T, ref1[3]),
                          cycle1_W_rel_diff=R.rel_diff(r1["W"], ref1[0]))), flush=True)


if __name__ == "__main__":
    main()
