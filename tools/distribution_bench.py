#!/usr/bin/env python3
"""tools/distribution_bench.py -- the distribution diagnostics on the GPU path (csrc/ops_distribution.hip).
Workloads:
  pbmc3k  (tests/golden/pbmc3k.spz, 13 714 x 2 700): an NB fit (k = 10, fp64), then score_test_distribution, diagnose_zero_inflation
          and diagnose_dispersion end to end (best of three after a warm-up); --cpu also times the numpy restatement
          (tests/distribution_ref.py) once, labelled as the CPU reference (it is not R's time).
  c5      simulate_nb_counts(10 000, 200 000, k = 32, density 0.02): 2e9 entries, a random fp64 model of rank 32; the zero-inflation
          and dispersion entries end to end.  The mu pass is 2 k m n flops (+ m n exponentials in the zero-inflation epilogue);
          each selection pass reads the 8 m n bytes of phi.  Kernel times come from a separate
          `rocprofv3 --kernel-trace --stats` run of this script (--only c5 --reps 1); the achieved rates are computed from them.
Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, data  # noqa: E402
from rcppml_amd import distribution as D  # noqa: E402


def best_of(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def pbmc3k(args):
    from oracle import oracle as O
    from rcppml_amd import nmf as N
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))
    t = time.perf_counter()
    model = N.nmf(A, 10, loss="nb", precision="fp64", seed=1, maxit=20)
    fit_s = time.perf_counter() - t
    out = dict(workload="pbmc3k", m=m, n=n, nnz=A.nnz, k=10, fit_nb_s=round(fit_s, 3))
    for name, f in (("score_test", lambda: D.score_test_distribution(A, model)),
                    ("zero_inflation", lambda: D.diagnose_zero_inflation(A, model)),
                    ("dispersion", lambda: D.diagnose_dispersion(A, model))):
        out[name + "_ms"] = round(best_of(f, args.reps) * 1e3, 3)
    out["all_three_ms"] = round(out["score_test_ms"] + out["zero_inflation_ms"] + out["dispersion_ms"], 3)
    r = D.diagnose_dispersion(A, model)
    out.update(dispersion_mode=r["mode"], zi_mode=D.diagnose_zero_inflation(A, model)["zi_mode"],
               best_distribution=D.score_test_distribution(A, model)["best_distribution"])
    if args.cpu:
        import distribution_ref as R
        Asp = A.to_scipy()
        t = time.perf_counter()
        R.score_test(Asp, model)
        R.zero_inflation(Asp, model)
        R.dispersion(Asp, model)
        out["numpy_restatement_all_three_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    return out


def c5(args):
    A, _, _ = data.simulate_nb_counts(10000, 200000, 32, density=0.02, seed=123)
    m, n, k = A.rows, A.cols, 32
    g = np.random.default_rng(5)
    W = g.uniform(0, 1, (m, k))
    d = np.ones(k)
    H = g.uniform(0, 1, (n, k)) * (5.0 / (0.25 * k))
    out = dict(workload="c5", m=m, n=n, nnz=A.nnz, k=k, entries=m * n, mu_pass_flops=2 * k * m * n, phi_bytes=8 * m * n)
    zi = lambda: _abi.zero_inflation_double(A, None, m, n, k, W, d, H)          # noqa: E731
    ds = lambda: _abi.dispersion_double(A, None, m, n, k, W, d, H, 1.0)         # noqa: E731
    r = zi()
    assert r["status"] == 0, r["error"]
    r = ds()
    assert r["status"] == 0, r["error"]
    out["zero_inflation_ms"] = round(best_of(zi, args.reps - 1) * 1e3, 2) if args.reps > 1 else None
    out["dispersion_ms"] = round(best_of(ds, args.reps - 1) * 1e3, 2) if args.reps > 1 else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("pbmc3k", "c5"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement on pbmc3k")
    args = ap.parse_args()
    for name, f in (("pbmc3k", pbmc3k), ("c5", c5)):
        if args.only in (None, name):
            print(json.dumps(f(args)), flush=True)


if __name__ == "__main__":
    main()
