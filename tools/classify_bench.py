#!/usr/bin/env python3
"""tools/classify_bench.py -- classifier evaluation on the GPU path (csrc/ops_classify.hip).
Workload: pbmc3k (tests/golden/pbmc3k.spz) with the embedding and labels of tools/assess_bench.py: the cell embedding v * d of
pca(k = 10) and the dclust(min_samples = 100) leaves.  Times, after one warm-up call each, the best of three end-to-end calls of
classify_embedding(k = 5), classify_logistic and classify_cv (5 folds, kNN k = 15 and logistic; split, host copies, upload, every
kernel and the host metrics included), with the kernel launches of each, and the numpy float64 restatement (tests/classify_ref.py)
once on the same input and the same split.  Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from rcppml_amd import _abi, classify as K  # noqa: E402


def best_of(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, min(ts)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def main():
    import assess_bench
    import classify_ref as CR
    X, lab, C, _, _ = assess_bench.pbmc3k()
    n, dim = X.shape
    knn, t_knn = best_of(lambda: K.classify_embedding(X, lab, k=5, seed=1))
    lr, t_lr = best_of(lambda: K.classify_logistic(X, lab, seed=1))
    cv, t_cv = best_of(lambda: K.classify_cv(X, lab, n_folds=5, k_nn=15, seed=42))
    tr, te = knn["train_idx"], knn["test_idx"]
    rk, c_knn = timed(lambda: CR.knn(X[tr], X[te], lab[tr], lab[te], C, 5))
    rl, c_lr = timed(lambda: CR.logistic(X[tr], X[te], lab[tr], lab[te], C))
    rc, c_cv = timed(lambda: CR.classify_cv(X, lab, C, cv["fold_ids"], 5))
    cv_launches = 0
    for fold in range(5):                                   # the launches of the ten entry calls of classify_cv
        test = cv["fold_ids"] == fold
        a, b = K.fold_scale(X[~test], X[test])
        cv_launches += _abi.classify_knn(a, b, lab[~test], lab[test], C, 15)["launches"]
        cv_launches += _abi.classify_logistic(a, b, lab[~test], lab[test], C)["launches"]
    rec = dict(workload="pbmc3k pca10 dclust", n=n, dim=dim, n_classes=C, n_test=len(te),
               classify_embedding_k5=dict(wall_s=t_knn, launches=knn["launches"], accuracy=knn["accuracy"], auc=knn["auc"],
                                          numpy_s=c_knn, predictions_equal_numpy=float(np.mean(rk["predictions"] == np.searchsorted(np.unique(lab), knn["predictions"])))),
               classify_logistic=dict(wall_s=t_lr, launches=lr["launches"], iters=lr["iters"].tolist(), accuracy=lr["accuracy"],
                                      auc=lr["auc"], numpy_s=c_lr, max_prob_diff_numpy=float(np.abs(rl["prob"] - lr["prob"]).max())),
               classify_cv=dict(wall_s=t_cv, launches=cv_launches, metrics=cv["metrics"], numpy_s=c_cv,
                                max_detail_diff_numpy=float(max(abs(d[m] - e[m]) for d, e in zip(cv["details"], rc) for m in K.CV_METRICS))),
               numpy_label="numpy float64 restatement (tests/classify_ref.py), one run, not the reference's R code")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
