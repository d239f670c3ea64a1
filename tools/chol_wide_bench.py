#!/usr/bin/env python3
"""Blocked Cholesky + clip (kernels_chol_wide.hip.h) at the ranks it opens, next to the CD solve on the same G and B with the
fit's defaults (cold start, cd_maxit = 100, cd_tol = 1e-8): one JSON line.

Per (dtype, k, ncols): chol_ms = rcppml_hip_solve_chol (factor + solve); factor_ms = the same call on ONE column (the factor
kernel plus a single-tile solve); solve_ms = chol_ms - factor_ms; cd_ms = rcppml_hip_solve_cd.  Device events around `reps`
back-to-back calls (reps / 5 for CD) after a warm-up call, the median of three such windows; reps = argv[1], default 50."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rcppml_amd import _abi

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return float(np.median(out))


def main():
    ctx = _abi.Context(0)
    rows = []
    for name, dt, td, ks in (("fp64", _abi.F64, torch.float64, (96, 160, 256)), ("fp32", _abi.F32, torch.float32, (160, 256))):
        for k in ks:
            rng = np.random.default_rng(k)
            F = rng.uniform(size=(4 * k + 5, k))
            G = torch.from_numpy(F.T @ F + 0.5 * np.eye(k)).to(td).cuda()
            for n in (2700, 13714):
                B = torch.from_numpy(3 * rng.standard_normal((n, k)) + 1).to(td).cuda()
                X = torch.zeros_like(B)
                chol = timed(lambda: ctx.solve_chol(dt, G, B, X, k, n, l1_pre=0.0, nonneg=1), REPS)
                factor = timed(lambda: ctx.solve_chol(dt, G, B, X, k, 1, l1_pre=0.0, nonneg=1), REPS)
                cd = timed(lambda: ctx.solve_cd(dt, G, B, X, k, n, l1_pre=0.0, warm=0, zero_init=1, nonneg=1, maxit=100, tol=1e-8,
                                                variant=_abi.CD_AUTO), max(1, REPS // 5))
                rows.append(dict(dtype=name, k=k, ncols=n, chol_ms=round(chol, 4), factor_ms=round(factor, 4),
                                 solve_ms=round(chol - factor, 4), cd_ms=round(cd, 4)))
    print(json.dumps(dict(bench="chol_wide", device=torch.cuda.get_device_name(0), reps=REPS, rows=rows)))


if __name__ == "__main__":
    main()
