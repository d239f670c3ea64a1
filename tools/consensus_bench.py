#!/usr/bin/env python3
"""tools/consensus_bench.py -- consensus clustering on the GPU path (rcppml_gpu_consensus_double, csrc/ops_consensus.hip).
Workload: pbmc3k cells (tests/golden/pbmc3k.spz transposed: 2 700 samples x 13 714 genes), k = 10, reps = 50, both methods, knn = 10.
Printed separately, each the median of --repeat (default 5) runs after one warm-up: the 50 nmf() fits (once: they do not depend on
the method), the consensus stage on the device (the entry end to end: upload of the W stack, kernels, download of the m x m result),
the host tree (rcppml_gpu_hclust_average_double), and the numpy / scipy restatement (tests/consensus_ref.py) of the consensus stage
on the same W stack (the CPU reference of the tests, not R's time; --ref-repeat runs, default 1).  One JSON line per method."""
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


def pbmc3k_cells():
    from oracle import oracle as O
    buf = np.fromfile(os.path.join(ROOT, "tests", "golden", "pbmc3k.spz"), dtype=np.uint8)
    _, m, n, _, _ = O.spz_info(buf)
    p, i, x = O.spz_decode(buf)
    A = sp.csc_matrix((np.asarray(x, np.float64), np.asarray(i), np.asarray(p)), shape=(m, n))
    return A.T.tocsc()                                   # samples = rows


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--knn", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--ref-repeat", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    if not _abi.detect():
        raise SystemExit("consensus_bench needs a GPU")
    import consensus_ref as R
    A = pbmc3k_cells()
    m = A.shape[0]

    def fits():
        return [nmf_module.nmf(A, args.k, seed=args.seed + i, verbose=False) for i in range(1, args.reps + 1)]

    models, t_fits = median_of(fits, args.repeat)
    W = np.stack([np.asarray(mod.w, np.float64) for mod in models])
    for method in ("hard", "knn_jaccard"):
        r, t_cons = median_of(lambda: _abi.consensus_double(W, m, args.k, args.reps, method, knn=args.knn), args.repeat)
        assert r["status"] == 0, r["error"]
        D = 1.0 - r["consensus"]
        t, t_tree = median_of(lambda: _abi.hclust_average_double(D, args.k), args.repeat)
        assert t["status"] == 0, t["error"]
        ref, t_ref = median_of(lambda: R.consensus(list(W), method, args.knn), args.ref_repeat)
        total = t_fits + t_cons + t_tree
        print(json.dumps(dict(workload="pbmc3k cells", m=m, n=A.shape[1], k=args.k, reps=args.reps, method=method,
                              knn=args.knn if method == "knn_jaccard" else None, fits_s=t_fits, consensus_device_s=t_cons,
                              tree_host_s=t_tree, total_s=total, consensus_share=t_cons / total, tree_share=t_tree / total,
                              restatement_consensus_s=t_ref, restatement_label="numpy / scipy restatement (tests/consensus_ref.py), "
                              "not the reference's code", bitwise_equal_to_restatement=bool(np.array_equal(ref, r["consensus"])),
                              cophenetic=t["cophenetic"], cluster_sizes=np.bincount(t["clusters"])[1:].tolist())), flush=True)


if __name__ == "__main__":
    main()
