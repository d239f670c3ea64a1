#!/usr/bin/env python3
"""tools/cluster_bench.py -- dclust() on the GPU clustering path (rcppml_gpu_dclust_ex, csrc/ops_cluster.hip).

Workloads: all of pbmc3k (tests/golden/pbmc3k.spz, 13714 x 2700, min_samples 100) and the BASELINE configs[1] matrix
(simulateNMF 20000 x 100000, k = 64, 1 %-dense, min_samples 1000).  Per workload, after one warm-up call: wall time of the whole
entry call (host CSC checks, upload, every level, leaf centers; the entry ends in a device synchronise), tree levels, splits,
rank-2 ALS iterations summed over splits, batched iterations (per level the slowest cluster's count rounded up to the poll
window of 8, summed over levels -- the launches the host issued), us per batched iteration, and a byte model of one batched
iteration divided by its time against the 6.3 TB/s measured copy rate.

Byte model (per level, per batched iteration; nnz_L = nonzeros of the level's clusters, C clusters, m rows):
  H pass   CSC of the level (12 B / nonzero + 4 B / column) + W_c gathered per nonzero (16 B)
  W pass   CSR of the level (12 B / nonzero) + h gathered per nonzero (16 B)
  finish   Wb read twice and W read + written, Wb zeroed: 5 x 16 B x m per cluster
These are logical bytes: every gather is counted at full size although much of it hits in L2 / MALL, and the time divided into them
is the whole call's (setup, polls and leaf centers included), so the rate is a coarse figure, not a roofline fraction.  --cpu also times the numpy restatement of the reference's CPU path (tests/cluster_ref.py) on pbmc3k: that is a
numpy restatement running on the machine's BLAS threads, not the reference's C++.  Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rcppml_amd import _abi, data  # noqa: E402

COPY_TBPS = 6.3
POLL = 8


def pbmc3k():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    st, m, n, nnz, vt = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    return data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))


def c2():
    import torch
    A, _, _ = data.simulate_nmf_sparse(20000, 100000, 64, 0.01, seed=123, device=torch.device("cuda", 0))
    return A


def tree_stats(A, r):
    """levels, splits, summed iterations, batched iterations and the byte model from the returned split tree."""
    N = r["nodes"]
    parent, it = r["parent"], r["iter"]
    depth = np.zeros(N, np.int64)
    for k in range(1, N):
        depth[k] = depth[parent[k]] + 1
    # nonzeros of every node: its leaves' columns, summed up the tree (children come after their parent)
    colnnz = np.diff(A.p).astype(np.int64)
    node_nnz = np.zeros(N, np.int64)
    for c in range(r["clusters"]):
        node_nnz[r["node"][c]] = colnnz[r["assignments"] == c].sum()
    for k in range(N - 1, 0, -1):
        node_nnz[parent[k]] += node_nnz[k]
    split = it >= 0
    levels = sorted(set(depth[split].tolist()))
    batched, bytes_total = 0, 0.0
    for L in levels:
        sel = split & (depth == L)
        b = int(np.ceil(it[sel].max() / POLL) * POLL)
        batched += b
        nnzL, C = float(node_nnz[sel].sum()), int(sel.sum())
        per_iter = nnzL * (12 + 16) + nnzL * (12 + 16) + 5 * 16.0 * A.rows * C
        bytes_total += b * per_iter
    return dict(levels=len(levels), splits=int(split.sum()), iterations=int(it[split].sum()), batched_iterations=batched,
                model_bytes=bytes_total)


def run(name, A, min_samples, reps, cpu):
    kw = dict(min_samples=min_samples, min_dist=0.0, seed=0.0)
    r = _abi.dclust_ex(A.p, A.i, A.x, A.rows, A.cols, **kw)           # warm-up (module load, first allocations)
    if r["status"] != 0:
        raise SystemExit("dclust failed: %s" % r["error"])
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = _abi.dclust_ex(A.p, A.i, A.x, A.rows, A.cols, **kw)
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    s = tree_stats(A, r)
    out = dict(workload=name, m=A.rows, n=A.cols, nnz=A.nnz, min_samples=min_samples, clusters=r["clusters"], wall_s=t,
               wall_s_all=ts, **s)
    out["us_per_batched_iteration"] = 1e6 * t / max(s["batched_iterations"], 1)
    out["model_TBps"] = s["model_bytes"] / t / 1e12
    out["model_fraction_of_copy_rate"] = out["model_TBps"] / COPY_TBPS
    if cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import cluster_ref as R
        t0 = time.perf_counter()
        cl = R.dclust(A.to_scipy(), min_samples=min_samples, seed=0)
        out["cpu_numpy_restatement_s"] = time.perf_counter() - t0
        out["cpu_label"] = "numpy restatement of the reference CPU path (tests/cluster_ref.py), not the reference's C++"
        out["cpu_same_tree"] = [c["id"] for c in cl] == r["ids"]
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=["pbmc3k", "c2", "all"], default="all")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement on pbmc3k")
    a = ap.parse_args()
    if a.workload in ("pbmc3k", "all"):
        run("pbmc3k", pbmc3k(), 100, a.reps, a.cpu)
    if a.workload in ("c2", "all"):
        run("configs[1] simulateNMF 20000x100000 1%", c2(), 1000, a.reps, False)


if __name__ == "__main__":
    main()
