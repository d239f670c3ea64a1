#!/usr/bin/env python3
"""tools/classify_rf_bench.py -- the histogram random forest on the GPU path (csrc/ops_classify_rf.hip).
Workload: the pbmc3k embedding and labels of tools/classify_bench.py (2 700 x 10, the dclust leaves as classes), the seed-1 split,
ntree = 500, default mtry.  Times, after one warm-up call, the best of three end-to-end calls of classify_rf() (split, host copies,
upload, every kernel, the per-level counter reads and the host metrics included), and reports the launches and the entry's own
host-side clock per stage and per tree level of the last call.  The numpy restatement (tests/classify_rf_ref.py) runs once at
ntree = --ref-trees on the same split; its time is scaled linearly to 500 trees and labelled as scaled.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from rcppml_amd import _abi, classify as K  # noqa: E402


def main():
    import assess_bench
    import classify_rf_ref as RF
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntree", type=int, default=500)
    ap.add_argument("--ref-trees", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    X, lab, C, _, _ = assess_bench.pbmc3k()
    n, dim = X.shape
    run = lambda: K.classify_rf(X, lab, ntree=args.ntree, seed=1)          # noqa: E731
    run()
    walls = []
    for _ in range(args.reps):                                             # every call ends in the entry's stream synchronise
        t0 = time.perf_counter()
        out = run()
        walls.append(time.perf_counter() - t0)
    # a size the embeddings of a large atlas reach: blobs, 100 000 x 32, 20 classes, 100 trees; one warm-up call, three timed
    import classify_ref as CR
    bx, bl = CR.blobs(100000, 32, 20, 0.7, 1)
    big = lambda: K.classify_rf(bx, bl, ntree=100, seed=1)                 # noqa: E731
    big()
    big_walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        big_out = big()
        big_walls.append(time.perf_counter() - t0)
    tr, te = out["train_idx"], out["test_idx"]
    codes = np.searchsorted(np.unique(lab), lab)
    raw = _abi._check(_abi.classify_rf(X[tr], X[te], codes[tr], codes[te], C, args.ntree, out["mtry"], 1), "classify_rf")
    levels = raw["ms"]["levels"]
    t0 = time.perf_counter()
    ref = RF.forest(X[tr], X[te], codes[tr], C, args.ref_trees, out["mtry"], seed=1)
    t_ref = time.perf_counter() - t0
    small = _abi._check(_abi.classify_rf(X[tr], X[te], codes[tr], codes[te], C, args.ref_trees, out["mtry"], 1), "classify_rf")
    rec = dict(workload="pbmc3k pca10 dclust", n=n, dim=dim, n_classes=C, n_train=len(tr), n_test=len(te), ntree=args.ntree,
               mtry=out["mtry"], wall_s=min(walls), wall_s_median=float(np.median(walls)), wall_s_max=max(walls), calls=len(walls),
               launches=out["launches"], accuracy=out["accuracy"], auc=out["auc"],
               blobs_100000x32_c20_ntree100=dict(wall_s=min(big_walls), wall_s_all=big_walls, launches=big_out["launches"],
                                                 mtry=big_out["mtry"], accuracy=big_out["accuracy"]),
               entry_ms=dict(setup_and_bootstrap=raw["ms"]["setup"], predict=raw["ms"]["predict"], levels_total=float(levels.sum()),
                             per_level=[round(float(v), 4) for v in levels[:int(np.flatnonzero(levels)[-1]) + 1]]),
               numpy=dict(ntree=args.ref_trees, wall_s=t_ref, scaled_to_ntree_s=t_ref * args.ntree / args.ref_trees,
                          votes_equal_device=bool(np.array_equal(ref["votes"], small["votes"])),
                          label="numpy restatement (tests/classify_rf_ref.py) at ntree = %d, one run, scaled linearly to %d trees; "
                                "not the reference's randomForest" % (args.ref_trees, args.ntree)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
