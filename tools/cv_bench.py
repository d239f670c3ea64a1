#!/usr/bin/env python3
"""Timing of the cross-validation half-updates (speckled mask, per-column Gram correction) at bench scale through the
device-level C ABI: H side and W side, zeros held out (the reference's default) or not.
usage: cv_bench.py [m [n [k]]] [--dtype f32|f64] [--repeats R]   (one line per case: the median, then every repeat)"""
import argparse, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rcppml_amd import als, data
ap = argparse.ArgumentParser()
ap.add_argument("m", type=int, nargs="?", default=20000)
ap.add_argument("n", type=int, nargs="?", default=100000)
ap.add_argument("k", type=int, nargs="?", default=32)
ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
ap.add_argument("--repeats", type=int, default=1)
args = ap.parse_args()
m, n, k = args.m, args.n, args.k
A, _, _ = data.simulate_nmf_sparse(m, n, k, 0.0115, seed=123, device=torch.device("cuda", 0))
At = A.transpose()
ops = als.HipOps(0, args.dtype)
W0, H0 = data.init_factors(42, k, m, n, ops.ndtype)
W, H = ops.to_device(W0), ops.to_device(H0)
Ad, Atd = ops.upload_csc(A), ops.upload_csc(At)
print("A %d x %d nnz %d k %d %s" % (m, n, A.nnz, k, args.dtype))
for mz in (1, 0):
    for solver in (0, 1):
        for name, csc, F, X, nrows, tr in (("H", Ad, W, H, m, 0), ("W", Atd, H, W, n, 1)):
            G = ops.gram(F, 2e-15, 0.1)
            Xc = X.clone()
            def run():
                ops.ctx.solve_cv(ops.dt, csc["p"], csc["i"], csc["x"], csc["cols"], nrows, F, G, Xc, k, 0.1, 7, mask_zeros=mz, transposed=tr,
                                 cd_maxit=100, solver_mode=solver)
            run(); torch.cuda.synchronize()
            ms = []
            for _ in range(args.repeats):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record(); run(); e.record(); torch.cuda.synchronize()
                ms.append(s.elapsed_time(e))
            print("cv %s mask_zeros=%d solver=%s: %.2f ms%s" % (name, mz, "cd" if solver == 0 else "chol", float(np.median(ms)),
                                                              "" if len(ms) == 1 else "  [" + " ".join("%.2f" % v for v in ms) + "]"))
