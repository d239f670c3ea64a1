"""numpy float64 restatement of the classifier evaluation: the spec of rcppml_amd/classify.py and csrc/ops_classify.hip.

Restated from the reference's R/classifier_metrics.R (classify_embedding :49-138, classify_logistic :219-291, .build_eval_result
:387-462, .compute_auc :469-492) and R/assess.R (.cv_classify :514-576, .compute_clf_metrics :655-695).  The GLM is written from the
algorithm of R's glm.fit for binomial(link = "logit") with unit prior weights (start mu = (y + 0.5) / 2, the C-level logit linkinv /
mu.eta with their +-30 thresholds, deviance 2 sum(-log mu or -log(1 - mu)), convergence |dev - devold| / (|dev| + 0.1) < epsilon).
R is not installed where this was written, so the restatement was NOT run against R; a prototype of it agreed with an unpenalised
maximum-likelihood fit to 1.7e-8 on a converging case.

Two least-squares solvers:
  "qr"    least squares on sqrt(W) X by Householder QR, as R's Cdqrls does (without its column pivoting: full-rank inputs only)
  "gram"  normal equations X'WX beta = X'Wz by a right-looking Cholesky; a pivot <= 1e-11 x the largest diagonal entry marks the
          column aliased (coefficient 0, its row and column skipped) -- the device's arithmetic, and how R drops the later of two
          collinear columns.

Measured gram - qr gap (max |prob difference| on the test rows; tests/test_classify_cpu.py::test_gram_against_qr prints it):
the six overlapping-blob cases <= 2.6e-15 (beta relative <= 2.7e-14); the four separable cases (25 iterations, not converged,
cond(X'WX) 1.3e3 to 6.9e3) 5.8e-15 to 2.8e-9.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
PIVOT_TOL = 1e-11


# ------------------------------------------------------------------------------------------------------------ metrics
def auc(y_true, scores):
    """.compute_auc: the literal loop over the stable descending order."""
    y_true = np.asarray(y_true)
    n = len(y_true)
    n_pos = int(np.sum(y_true == 1))
    n_neg = n - n_pos
    if n == 0 or n_pos == 0 or n_neg == 0:
        return 0.5
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    tp, total = 0, 0
    for i in order:
        if y_true[i] == 1:
            tp += 1
        else:
            total += tp
    return total / (n_pos * n_neg)


def which_max(row):
    return int(np.argmax(row))          # first maximum, as R's which.max


def metrics(pred, truth, prob, C):
    """.build_eval_result on codes 0 .. C - 1."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    conf = np.zeros((C, C), np.int64)
    for t, p in zip(truth, pred):
        conf[t, p] += 1
    prec, rec, f1, sup = np.zeros(C), np.zeros(C), np.zeros(C), np.zeros(C, np.int64)
    for c in range(C):
        tp = conf[c, c]
        fp = conf[:, c].sum() - tp
        fn = conf[c, :].sum() - tp
        prec[c] = tp / (tp + fp) if tp + fp > 0 else 0.0
        rec[c] = tp / (tp + fn) if tp + fn > 0 else 0.0
        f1[c] = 2 * prec[c] * rec[c] / (prec[c] + rec[c]) if prec[c] + rec[c] > 0 else 0.0
        sup[c] = conf[c, :].sum()
    aucs = np.array([auc((truth == c).astype(int), prob[:, c]) for c in range(C)])
    return dict(predictions=pred.astype(np.int64), confusion=conf, precision=prec, recall=rec, f1=f1, support=sup, auc=aucs,
                accuracy=float(np.sum(pred == truth)) / len(truth), macro_precision=prec.mean(), macro_recall=rec.mean(),
                macro_f1=f1.mean(), weighted_f1=float(np.sum(f1 * sup)) / max(int(sup.sum()), 1), macro_auc=aucs.mean())


def clf_metrics(m):
    """.compute_clf_metrics: the five figures of one fold."""
    return dict(accuracy=m["accuracy"], f1=m["macro_f1"], precision=m["macro_precision"], recall=m["macro_recall"],
                auroc=m["macro_auc"])


# ------------------------------------------------------------------------------------------------------------ kNN
def knn(train, test, ltr, lte, C, k, distance="euclidean"):
    """classify_embedding's loop in float64.  Also returns the neighbours and, per test row, the relative gap between the k-th and
    the (k + 1)-th distance (inf when k = n_train)."""
    train, test = np.asarray(train, np.float64), np.asarray(test, np.float64)
    if distance == "cosine":
        def unit(a):
            nrm = np.sqrt(np.sum(a * a, axis=1))
            nrm[nrm == 0] = 1
            return a / nrm[:, None]
        train, test = unit(train), unit(test)
    nt = test.shape[0]
    votes = np.zeros((nt, C))
    pred = np.zeros(nt, np.int64)
    nn = np.zeros((nt, k), np.int64)
    gap = np.full(nt, np.inf)
    for i in range(nt):
        d = np.sum((train - test[i]) ** 2, axis=1)
        o = np.argsort(d, kind="stable")
        nn[i] = o[:k]
        if k < len(d):
            gap[i] = (d[o[k]] - d[o[k - 1]]) / max(d[o[k]], np.finfo(float).tiny)
        cnt = np.bincount(np.asarray(ltr)[o[:k]], minlength=C)
        votes[i] = cnt / k
        pred[i] = which_max(cnt)
    out = metrics(pred, lte, votes, C)
    out.update(votes=votes, nn=nn, gap=gap)
    return out


# ------------------------------------------------------------------------------------------------------------ GLM
def linkinv(eta):
    t = np.where(eta < -30, EPS, np.where(eta > 30, 1 / EPS, np.exp(np.clip(eta, -30, 30))))
    return t / (1 + t)


def mu_eta(eta):
    ae = np.abs(eta)
    ex = np.exp(-np.minimum(ae, 30))
    return np.where(ae > 30, EPS, np.maximum(ex / (1 + ex) ** 2, EPS))


def deviance(y, mu):
    om = 1 - mu
    return 2 * np.sum(np.where(y == 1, -np.log(mu), -np.log(om)))


def chol_solve(A, b):
    """Right-looking Cholesky with the pivot rule; returns (beta, aliased, the smallest kept pivot / the largest diagonal entry).
    Roundoff in the solve is amplified by the reciprocal of that ratio."""
    A = np.array(A, np.float64)
    P = A.shape[0]
    floor = PIVOT_TOL * np.max(np.diag(A))
    al = np.zeros(P, bool)
    L = np.zeros((P, P))
    ratio = np.inf
    for j in range(P):
        piv = A[j, j]
        if not piv > floor:
            al[j] = True
            continue
        ratio = min(ratio, piv / (floor / PIVOT_TOL))
        ljj = np.sqrt(piv)
        L[j, j] = ljj
        L[j + 1:, j] = A[j + 1:, j] / ljj
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    keep = np.flatnonzero(~al)
    Lk = L[np.ix_(keep, keep)]
    y = np.zeros(len(keep))
    for a in range(len(keep)):
        y[a] = (b[keep[a]] - Lk[a, :a] @ y[:a]) / Lk[a, a]
    x = np.zeros(len(keep))
    for a in range(len(keep) - 1, -1, -1):
        x[a] = (y[a] - Lk[a + 1:, a] @ x[a + 1:]) / Lk[a, a]
    beta = np.zeros(P)
    beta[keep] = x
    return beta, al, ratio


def glm_binomial(X, y, maxit=25, epsilon=1e-8, solver="gram"):
    """glm.fit for binomial(logit), unit weights.  X holds the intercept column.  Returns dict(beta, aliased, iters, converged,
    deviance, ratios (the convergence ratio of every iteration), cond (of the last X'WX, non-aliased part), min_pivot (the
    smallest kept pivot ratio of chol_solve over the iterations; "gram" only))."""
    y = np.asarray(y, np.float64)
    mu = (y + 0.5) / 2
    eta = np.log(mu / (1 - mu))
    devold = deviance(y, mu)
    ratios, conv, beta, al, cond, min_pivot = [], False, np.zeros(X.shape[1]), np.zeros(X.shape[1], bool), np.nan, np.inf
    it = 0
    for it in range(1, maxit + 1):
        g = mu_eta(eta)
        z = eta + (y - mu) / g
        w = g * g / (mu * (1 - mu))
        if solver == "gram":
            G = X.T @ (w[:, None] * X)
            beta, al, pr = chol_solve(G, X.T @ (w * z))
            min_pivot = min(min_pivot, pr)
            keep = ~al
            cond = np.linalg.cond(G[np.ix_(keep, keep)]) if keep.any() else np.nan
        else:
            sw = np.sqrt(w)
            Q, R = np.linalg.qr(sw[:, None] * X)
            beta = np.linalg.solve(R, Q.T @ (sw * z))
            cond = np.linalg.cond(R) ** 2
        eta = X @ beta
        mu = linkinv(eta)
        dev = deviance(y, mu)
        ratios.append(abs(dev - devold) / (abs(dev) + 0.1))
        if ratios[-1] < epsilon:
            conv = True
            break
        devold = dev
    return dict(beta=beta, aliased=al.astype(np.int64), iters=it, converged=int(conv), deviance=dev, ratios=ratios, cond=cond,
                min_pivot=min_pivot)


def logistic(train, test, ltr, lte, C, maxit=25, epsilon=1e-8, solver="gram"):
    """classify_logistic's one-vs-rest fits and row-normalised probabilities."""
    train, test = np.asarray(train, np.float64), np.asarray(test, np.float64)
    X = np.hstack([np.ones((train.shape[0], 1)), train])
    T = np.hstack([np.ones((test.shape[0], 1)), test])
    fits = [glm_binomial(X, (np.asarray(ltr) == c).astype(np.float64), maxit, epsilon, solver) for c in range(C)]
    prob = np.stack([linkinv(T @ f["beta"]) for f in fits], axis=1)
    s = prob.sum(axis=1)
    s[s == 0] = 1
    prob = prob / s[:, None]
    pred = np.array([which_max(r) for r in prob])
    out = metrics(pred, lte, prob, C)
    out.update(prob=prob, coef=np.stack([f["beta"] for f in fits]), aliased=np.stack([f["aliased"] for f in fits]),
               iters=np.array([f["iters"] for f in fits]), converged=np.array([f["converged"] for f in fits]),
               deviance=np.array([f["deviance"] for f in fits]), ratios=[f["ratios"] for f in fits],
               cond=np.array([f["cond"] for f in fits]), min_pivot=min(f["min_pivot"] for f in fits))
    return out


# ------------------------------------------------------------------------------------------------------------ cross-validation
def fold_scale(train, test):
    means = train.mean(axis=0)
    sds = train.std(axis=0, ddof=1)
    sds[sds == 0] = 1
    return (train - means) / sds, (test - means) / sds


def classify_cv(emb, codes, C, fold_ids, n_folds, classifiers=("knn", "lr"), k_nn=15):
    """.cv_classify given the fold ids (0-based): the details rows, fold outer, classifier inner."""
    emb, codes = np.asarray(emb, np.float64), np.asarray(codes)
    rows = []
    for fold in range(n_folds):
        test = fold_ids == fold
        if not test.any() or test.all():
            continue
        tr, te = fold_scale(emb[~test], emb[test])
        for clf in classifiers:
            if clf == "knn":
                m = knn(tr, te, codes[~test], codes[test], C, min(k_nn, tr.shape[0]))
            else:
                m = logistic(tr, te, codes[~test], codes[test], C)
            rows.append(dict(classifier=clf, fold=fold + 1, **clf_metrics(m)))
    return rows


# ------------------------------------------------------------------------------------------------------------ inputs
def blobs(n, p, C, spread, seed, labels=None):
    """Gaussian blobs with standardised columns: class centres N(0, spread^2) per coordinate, unit noise.  Returns (x, labels)."""
    rng = np.random.default_rng(seed)
    lab = np.arange(n) % C if labels is None else np.asarray(labels)
    rng.shuffle(lab)
    centres = rng.standard_normal((C, p)) * spread
    x = centres[lab] + rng.standard_normal((n, p))
    x = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
    return x, lab.astype(np.int32)
