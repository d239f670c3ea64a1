"""classify_embedding(), classify_logistic() and classify_cv(): host-side mirror of the reference's classifier evaluation
(R/classifier_metrics.R:49-138, 219-291, 387-492 and .cv_classify, R/assess.R:514-695) on the HIP classifier path
(csrc/ops_classify.hip).  The messages, the label factorisation, k = min(k, n - 1), the metric keys and the fold scaling are R's; the
computation is the three build-defined entries.  No CPU fallback: without a device the calls raise BackendError.

Deviations from R, all documented in DESIGN.md 4.14:
  * The random split is not R's Mersenne-Twister sample.int.  It is a partial Fisher-Yates shuffle on the project's SplitMix64
    stream: idx = 0 .. n - 1; for i = 0 .. n_test - 1: j = i + floor(u_i (n - i)) (capped at n - 1), swap idx[i] and idx[j], with
    u_i = draw i of data.splitmix64_uniform(seed); the test set is idx[:n_test].  seed=None means seed 0 (R would leave the
    session's RNG state alone; there is no session state here), which the project's stream, like the reference's rng, takes as
    12345.
  * Indices (test_idx, train_idx) are 0-based.
  * kNN distances are fp32; the logistic fit solves the normal equations by Cholesky where R's glm.fit uses QR.
  * predictions / test_labels hold the label values (levels[code]); R returns integer codes for a factor.
"""
import numpy as np

from . import _abi
from .assess import _embedding, _factor, _nanmean
from .data import splitmix64_uniform

DISTANCES = ("euclidean", "cosine")
CV_METRICS = ("accuracy", "f1", "precision", "recall", "auroc")


def split_indices(n, test_fraction=0.2, seed=None):
    """The test indices of the random split (0-based, in draw order): the partial Fisher-Yates rule of the module docstring."""
    n_test = max(1, int(round(n * test_fraction)))          # Python and R both round half to even
    n_test = min(n_test, n)
    u = splitmix64_uniform(0 if seed is None else int(seed), 0, n_test)
    idx = np.arange(n, dtype=np.int64)
    for i in range(n_test):
        j = min(i + int(np.floor(u[i] * (n - i))), n - 1)
        idx[i], idx[j] = idx[j], idx[i]
    return idx[:n_test].copy()


def _prepare(embedding, labels, test_fraction, test_idx, seed):
    emb = _embedding(embedding)
    n = emb.shape[0]
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("length(labels) must equal nrow(embedding)")
    levels, codes = _factor(labels)
    if test_idx is None:
        test_idx = split_indices(n, test_fraction, seed)
    else:
        test_idx = np.asarray(test_idx, dtype=np.int64).ravel()
        if test_idx.size < 1 or test_idx.min() < 0 or test_idx.max() >= n:
            raise ValueError("test_idx must hold indices in [0, nrow(embedding))")
    train_idx = np.setdiff1d(np.arange(n, dtype=np.int64), test_idx)
    return emb, levels, codes, train_idx, test_idx


def _eval_result(r, levels, codes, train_idx, test_idx, method):
    """.build_eval_result (classifier_metrics.R:387-462) from the entry's per-class results."""
    C = len(levels)
    support = r["support"].astype(np.int64)
    total = int(support.sum())
    test_codes = codes[test_idx]
    return dict(
        accuracy=float(np.sum(r["predictions"] == test_codes)) / len(test_idx),
        per_class={"class": levels.copy(), "precision": r["precision"], "recall": r["recall"], "f1": r["f1"], "support": support},
        macro_precision=float(np.mean(r["precision"])), macro_recall=float(np.mean(r["recall"])), macro_f1=float(np.mean(r["f1"])),
        weighted_f1=float(np.sum(r["f1"] * support)) / max(total, 1),
        auc=float(np.mean(r["auc"])), per_class_auc=r["auc"], confusion=r["confusion"],
        predictions=levels[r["predictions"]], test_labels=levels[test_codes], train_idx=train_idx, test_idx=test_idx, method=method,
        n_classes=C)


def classify_embedding(embedding, labels, test_fraction=0.2, test_idx=None, k=5, seed=None, distance="euclidean"):
    """kNN classifier on an embedding, evaluated on held-out rows (R's classify_embedding).  embedding: a matrix (rows are samples)
    or anything assess() accepts.  Returns R's fn_classifier_eval fields as a dict, plus k and distance."""
    if distance not in DISTANCES:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % d for d in DISTANCES))
    emb, levels, codes, train_idx, test_idx = _prepare(embedding, labels, test_fraction, test_idx, seed)
    k = int(min(k, emb.shape[0] - 1))
    if len(train_idx) < k:
        raise ValueError("Fewer training samples than k neighbors")
    r = _abi._check(_abi.classify_knn(emb[train_idx], emb[test_idx], codes[train_idx], codes[test_idx], len(levels), k, distance),
                    "classify_embedding")
    out = _eval_result(r, levels, codes, train_idx, test_idx, "knn")
    out.update(k=k, distance=distance, votes=r["votes"], launches=r["launches"])
    return out


def classify_logistic(embedding, labels, test_fraction=0.2, test_idx=None, seed=None):
    """One-vs-rest logistic regression on an embedding, evaluated on held-out rows (R's classify_logistic: one binomial glm() per
    class, probabilities row-normalised).  Returns R's fn_classifier_eval fields as a dict, plus coef (C x (p + 1), intercept
    first), aliased, iters, converged, deviance (per class) and prob (n_test x C)."""
    emb, levels, codes, train_idx, test_idx = _prepare(embedding, labels, test_fraction, test_idx, seed)
    r = _abi._check(_abi.classify_logistic(emb[train_idx], emb[test_idx], codes[train_idx], codes[test_idx], len(levels)),
                    "classify_logistic")
    out = _eval_result(r, levels, codes, train_idx, test_idx, "logistic")
    out.update({key: r[key] for key in ("coef", "aliased", "iters", "converged", "deviance", "prob", "launches")})
    return out


def fold_scale(train, test):
    """R's scale() by the training columns' mean and sd (n - 1; an sd of 0 becomes 1)."""
    means = train.mean(axis=0)
    sds = train.std(axis=0, ddof=1) if train.shape[0] > 1 else np.full(train.shape[1], np.nan)
    sds = np.where(sds == 0, 1.0, sds)
    return (train - means) / sds, (test - means) / sds


def classify_cv(embedding, labels, n_folds=5, classifiers=("knn", "lr"), k_nn=15, seed=42):
    """Stratified k-fold classification (R's .cv_classify): per fold the embedding is scaled by the training mean and sd, then a
    kNN (k = min(k_nn, n_train)) and / or a one-vs-rest logistic classifier is fitted and scored.  The folds are those of assess()
    (the rcppml_gpu_assess_plan fold ids of `seed`).  Returns dict(details: one dict per (fold, classifier) with classifier, fold
    (1-based), accuracy, f1, precision, recall, auroc; metrics: the *_knn, *_lr and *_mean keys assess() forms; fold_ids).  Where
    R's tryCatch would record NA for a fold that fails, a failing fold raises here."""
    classifiers = [classifiers] if isinstance(classifiers, str) else list(classifiers)
    bad = [c for c in classifiers if c == "rf"]
    if bad:
        raise ValueError("classifiers %s run on R's CPU path and are not available here" % ", ".join('"%s"' % c for c in bad))
    unknown = [c for c in classifiers if c not in ("knn", "lr")]
    if unknown:
        raise ValueError("unknown classifier %s" % ", ".join('"%s"' % c for c in unknown))
    emb = _embedding(embedding)
    n = emb.shape[0]
    labels = np.asarray(labels)
    if labels.ndim != 1 or labels.shape[0] != n:
        raise ValueError("length(labels) must equal nrow(embedding)")
    if int(n_folds) < 1:
        raise ValueError("n_folds must be >= 1")
    levels, codes = _factor(labels)
    C = len(levels)
    fold_ids = _abi._check(_abi.assess_plan(codes, C, nstart=0, spc=0, folds=int(n_folds), seed=seed), "fold plan")["fold_ids"]
    details = []
    for fold in range(int(n_folds)):
        test = fold_ids == fold
        if not test.any() or test.all():
            continue
        tr, te = fold_scale(emb[~test], emb[test])
        ytr, yte = codes[~test], codes[test]
        for clf in classifiers:
            if clf == "knn":
                r = _abi._check(_abi.classify_knn(tr, te, ytr, yte, C, min(int(k_nn), tr.shape[0])), "classify_cv (knn)")
            else:
                r = _abi._check(_abi.classify_logistic(tr, te, ytr, yte, C), "classify_cv (lr)")
            details.append(dict(classifier=clf, fold=fold + 1, accuracy=float(np.mean(r["predictions"] == yte)),
                                f1=float(np.mean(r["f1"])), precision=float(np.mean(r["precision"])),
                                recall=float(np.mean(r["recall"])), auroc=float(np.mean(r["auc"]))))
    return dict(details=details, metrics=cv_summary(details), fold_ids=fold_ids)


def cv_summary(details):
    """The keys assess() forms from the details rows: <metric>_<classifier> and <metric>_mean (NaN-skipping means)."""
    out = {}
    for clf in dict.fromkeys(d["classifier"] for d in details):
        rows = [d for d in details if d["classifier"] == clf]
        for m in CV_METRICS:
            out["%s_%s" % (m, clf)] = _nanmean([d[m] for d in rows])
    for m in CV_METRICS:
        out["%s_mean" % m] = _nanmean([d[m] for d in details])
    return out
