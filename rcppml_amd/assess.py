"""assess() and knn(): host-side mirror of the reference R surface (R/assess.R:61-196, the GPU branch) on the HIP assessment path
(csrc/ops_assess.hip).  Embedding extraction, label factorisation, the small-class filter, the messages and the metric keys are R's;
the computation is the 26-pointer entry with R's constants (10 k-means restarts of 100 iterations).  The "lr" and "rf" classifiers
run on R's CPU and are not provided here.  No CPU fallback: without a device the calls raise BackendError."""
import sys

import numpy as np

from . import _abi

ALL_METRICS = ("ari", "nmi", "silhouette", "classification", "batch_mixing")
KMEANS_NSTART, KMEANS_MAXITER = 10, 100          # R/assess.R:744-745


def _embedding(x):
    """R's .extract_embedding: a matrix as is; an nmf() result (dict with w, d, h) -> t(d * h); an svd()/pca() result (dict with u,
    d) -> u %*% diag(d)."""
    if isinstance(x, dict):
        if "h" in x:
            return (np.asarray(x["d"], np.float64)[:, None] * np.asarray(x["h"], np.float64)).T
        if "u" in x:
            return np.asarray(x["u"], np.float64) * np.asarray(x["d"], np.float64)[None, :]
        raise ValueError("x must be a matrix, an nmf() result or an svd()/pca() result")
    e = np.asarray(x, np.float64)
    if e.ndim != 2:
        raise ValueError("x must be a matrix, an nmf() result or an svd()/pca() result")
    return e


def _factor(v):
    """as.factor: sorted levels, 0-based codes."""
    levels, codes = np.unique(np.asarray(v), return_inverse=True)
    return levels, codes.astype(np.int32)


def _metrics(metrics, has_batch):
    if isinstance(metrics, str):
        metrics = [metrics]
    metrics = list(metrics)
    if len(metrics) == 1 and metrics[0] == "all":
        return [m for m in ALL_METRICS if has_batch or m != "batch_mixing"]
    out = []
    for m in metrics:
        hits = [a for a in ALL_METRICS if a.startswith(m)] if m else []
        if len(hits) != 1:
            raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % a for a in ALL_METRICS))
        if hits[0] not in out:
            out.append(hits[0])
    return out


def assess(x, labels, batch=None, metrics="all", n_folds=5, classifiers=("knn",), k_nn=15, seed=42, min_class_size=10,
           sil_samples_per_class=200, batch_knn_k=50):
    """Embedding quality on the GPU (R's assess() GPU branch).  Returns dict(metrics, classification, params) with R's metric keys:
    ari, nmi, silhouette, {accuracy,f1,precision,recall,auroc}_knn and _mean (precision / recall / AUROC NaN, as R's
    mean(NA, na.rm = TRUE)), batch_silhouette, batch_knn_entropy; params["backend"] = "gpu"."""
    emb = _embedding(x)
    n, k = emb.shape
    labels = np.asarray(labels)
    if labels.shape[0] != n:
        raise ValueError("length(labels) must equal nrow of embedding (%d)" % n)
    classifiers = [classifiers] if isinstance(classifiers, str) else list(classifiers)
    bad = [c for c in classifiers if c in ("lr", "rf")]
    if bad:
        raise ValueError("classifiers %s run on R's CPU path and are not available here" % ", ".join('"%s"' % c for c in bad))
    do = _metrics(metrics, batch is not None)
    levels, codes = _factor(labels)
    counts = np.bincount(codes, minlength=len(levels))
    keep = counts >= min_class_size
    if int(keep.sum()) < 2:
        raise ValueError("Fewer than 2 classes with >= %d samples" % min_class_size)
    mask = keep[codes]
    if batch is not None:
        batch = np.asarray(batch)
    if int((~mask).sum()) > 0:
        print("Dropped %d samples from %d small classes (min_class_size=%d)" % (int((~mask).sum()), len(levels) - int(keep.sum()),
                                                                               min_class_size), file=sys.stderr)
        emb = emb[mask]
        levels, codes = _factor(labels[mask])          # droplevels
        if batch is not None:
            batch = batch[mask]
        n = emb.shape[0]
    n_classes = len(levels)
    bcodes, n_batch = None, 0
    if batch is not None:
        blev, bcodes = _factor(batch)
        n_batch = len(blev)
    r = _abi.assess_raw(emb, codes, n_classes, bcodes if bcodes is not None else np.zeros(n, np.int32), n_batch,
                        clustering="ari" in do or "nmi" in do, silhouette="silhouette" in do, classify="classification" in do,
                        batch_mixing="batch_mixing" in do and n_batch > 1, nstart=KMEANS_NSTART, maxiter=KMEANS_MAXITER,
                        spc=sil_samples_per_class, knn_k=k_nn, folds=n_folds, batch_k=batch_knn_k, seed=seed)
    if r["status"] != 0:
        raise _abi.BackendError("GPU assess failed: %s" % r["error"])
    out = {}
    if "ari" in do:
        out["ari"] = r["ari"]
    if "nmi" in do:
        out["nmi"] = r["nmi"]
    if "silhouette" in do:
        out["silhouette"] = r["silhouette"]
    details = None
    if "classification" in do:
        details = []
        if "knn" in classifiers:
            details.append(dict(classifier="knn", fold=0, accuracy=r["knn_accuracy"], f1=r["knn_f1"], precision=np.nan,
                                recall=np.nan, auroc=np.nan))
        names = ("accuracy", "f1", "precision", "recall", "auroc")
        for clf in dict.fromkeys(d["classifier"] for d in details):
            rows = [d for d in details if d["classifier"] == clf]
            for m in names:
                out["%s_%s" % (m, clf)] = _nanmean([d[m] for d in rows])
        for m in names:
            out["%s_mean" % m] = _nanmean([d[m] for d in details])
    if "batch_mixing" in do and n_batch > 1:
        out["batch_silhouette"] = r["batch_sil"]
        out["batch_knn_entropy"] = r["batch_entropy"]
    params = dict(n_samples=n, n_features=k, n_classes=n_classes, metrics=do, n_folds=n_folds, classifiers=classifiers, k_nn=k_nn,
                  seed=seed, min_class_size=min_class_size, has_batch=batch is not None, backend="gpu")
    return dict(metrics=out, classification=details, params=params)


def _nanmean(v):
    """R's mean(x, na.rm = TRUE): NaN when nothing is left."""
    v = [float(a) for a in v if not np.isnan(a)]
    return float(np.mean(v)) if v else float("nan")


def knn(query, train=None, k=15, mask="none", group=None, group_k=None):
    """Exact fp32 brute-force kNN on the GPU: the k smallest candidates in (squared distance, index) order.  train None: the query
    matrix itself (mask "self" leaves each point out, mask "group" the points of its own group; group_k: k per group).  Returns
    (idx, dist): n_query x k, -1 / 1e30 for empty slots."""
    r = _abi.knn_float(query, train, int(k), mask=mask, group=group, group_k=group_k)
    if r["status"] != 0:
        raise _abi.BackendError("GPU kNN failed: %s" % r["error"])
    return r["idx"], r["dist"]
