#!/usr/bin/env python3
"""tools/assess_bench.py -- embedding assessment on the GPU path (rcppml_gpu_assess, csrc/ops_assess.hip).
Workloads:
  (a) pbmc3k (tests/golden/pbmc3k.spz): the cell embedding v * d of pca(k = 10), dclust(min_samples = 100) leaves as labels, a
      synthetic two-level batch (cell index mod 2), all metrics with R's constants (10 k-means restarts x 100 iterations, 200
      silhouette samples per class, k_nn 15, 5 folds, batch k 50);
  (b) Gaussian blobs, 100 000 x 32, 20 classes, 4 batches, the same metrics.
Per workload, after one warm-up call: the best of three end-to-end times of the 26-pointer entry (fp32 cast, upload, every metric,
host ARI / NMI / votes / entropy), the time of each metric alone (the flags one at a time), and the exact self-kNN's pair rate:
one knn call of k = 15 over all n points, pairs = n^2, against the unpacked fp32 bound of 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
= 39.3 T lane-ops/s at dim lane-ops (one fmaf each) per pair.  --cpu also times the numpy restatement (tests/assess_ref.py) of the
silhouette and the batch metrics on a 5 000-point subsample, labelled as such.  Prints one JSON line per workload."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from rcppml_amd import _abi, data  # noqa: E402

LANE_OPS = 256 * 4 * 16 * 2.4e9


def pbmc3k():
    from oracle import oracle as O
    from rcppml_amd import cluster, svd
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = data.CSC((m, n), np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64))
    pc = svd.pca(A, k=10, seed=1)
    labels = np.zeros(n, np.int32)
    for c, leaf in enumerate(cluster.dclust(A, min_samples=100, seed=1)):
        labels[leaf["samples"]] = c
    return pc["v"] * pc["d"][None, :], labels, int(labels.max()) + 1, (np.arange(n) % 2).astype(np.int32), 2


def blobs(n=100000, dim=32, K=20, B=4, seed=0):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-4, 4, (K, dim))
    lab = rng.integers(0, K, n).astype(np.int32)
    X = centers[lab] + rng.standard_normal((n, dim))
    return X, lab, K, rng.integers(0, B, n).astype(np.int32), B


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, min(ts)


def run(name, X, lab, K, batch, B, cpu):
    n, dim = X.shape
    kw = dict(nstart=10, maxiter=100, spc=200, knn_k=15, folds=5, batch_k=50, seed=42)
    flags = ("clustering", "silhouette", "classify", "batch_mixing")
    call = lambda on: _abi.assess_raw(X, lab, K, batch, B, **{f: f in on for f in flags}, **kw)
    r, t_all = best_of(lambda: call(flags))
    assert r["status"] == 0, r["error"]
    per = {}
    for f in flags:
        rr, per[f] = best_of(lambda: call((f,)))
        assert rr["status"] == 0, rr["error"]
    X32 = np.ascontiguousarray(X, np.float32)
    kr, t_knn = best_of(lambda: _abi.knn_float(X32, None, 15, mask="self"))
    assert kr["status"] == 0, kr["error"]
    pairs = float(n) * n
    rec = dict(workload=name, n=n, dim=dim, n_classes=K, n_batch=B, wall_s=t_all, metric_s=per,
               metrics={k: r[k] for k in ("ari", "nmi", "silhouette", "knn_accuracy", "knn_f1", "batch_sil", "batch_entropy")},
               knn_self_k15_s=t_knn, knn_pairs_per_s=pairs / t_knn, knn_lane_ops_per_s=pairs * dim / t_knn,
               knn_share_of_unpacked_bound=pairs * dim / t_knn / LANE_OPS)
    if cpu:
        import assess_ref as R
        sub = np.random.default_rng(1).choice(n, min(n, 5000), replace=False)
        Xs, ls, bs = X[sub].astype(np.float32), lab[sub], batch[sub]
        t0 = time.perf_counter()
        R.silhouette(Xs, ls, K, 200, 42)
        R.batch_mixing(Xs, bs, B, 50)
        rec["cpu_s_5000_points_sil_batch"] = time.perf_counter() - t0
        rec["cpu_label"] = "numpy restatement (tests/assess_ref.py) of silhouette + batch mixing on 5000 points, not the reference's code"
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement (slow)")
    ap.add_argument("--only", choices=("pbmc3k", "blobs"), default=None)
    args = ap.parse_args()
    if args.only in (None, "pbmc3k"):
        run("pbmc3k pca10 dclust", *pbmc3k(), args.cpu)
    if args.only in (None, "blobs"):
        run("blobs 100000x32", *blobs(), args.cpu)


if __name__ == "__main__":
    main()
