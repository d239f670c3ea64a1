"""numpy float64 / int64 restatement of the histogram forest: the complete specification of classify.classify_rf() and
csrc/ops_classify_rf.hip.  The device agrees with it exactly: every split, every vote.

Counts are integers; the only floating-point steps are the binning and the split score, each one fixed expression in float64.
  binning     v = (x - lo_f) * (256.0 / (hi_f - lo_f)); bin = 255 if v >= 255, floor(v) if v > 0, else 0; 0 when hi_f == lo_f
  draws       u_q = splitmix64_uniform(seed, q, 1)
  bootstrap   tree t, i < n: row min(floor(u_{t n + i} n), n - 1) gains one multiplicity
  candidates  node `node` of tree t: partial Fisher-Yates over 0 .. p - 1 with u_q, q = ntree n + (t 2n + node) p + i, i < mtry
  score       S_L / N_L + S_R / N_R over thresholds 0 .. 254 with N_L, N_R > 0; largest wins, ties to the smaller feature, then t
  leaves      pure, in-bag count < 2, no valid split, or depth 40; every node carries its majority class (ties to the smaller)
"""
import numpy as np

from rcppml_amd.data import splitmix64_uniform

MAX_DEPTH = 40


def bin_edges(train):
    return train.min(axis=0), train.max(axis=0)


def bins(x, lo, hi):
    span = hi - lo
    with np.errstate(all="ignore"):
        v = (x - lo) * (256.0 / span)
        b = np.where(v >= 255.0, 255.0, np.where(v > 0.0, np.floor(v), 0.0)).astype(np.int64)
    b[:, span == 0] = 0
    return b


def candidates(seed, q0, p, mtry):
    u = splitmix64_uniform(seed, q0, mtry)
    idx = list(range(p))
    for i in range(mtry):
        j = min(i + int(np.floor(u[i] * (p - i))), p - 1)
        idx[i], idx[j] = idx[j], idx[i]
    return sorted(idx[:mtry])


def best_split(b, y, w, C, feats):
    """(feature, threshold, N_L) of the best split of the rows given (bins b, classes y, multiplicities w), or None."""
    nbag, best = int(w.sum()), None
    for f in feats:
        hist = np.zeros((C, 256), np.int64)
        np.add.at(hist, (y, b[:, f]), w)
        L = np.cumsum(hist, axis=1)[:, :255]
        R = hist.sum(axis=1)[:, None] - L
        NL = L.sum(axis=0)
        ok = (NL > 0) & (NL < nbag)
        if not ok.any():
            continue
        with np.errstate(all="ignore"):
            score = (L * L).sum(axis=0).astype(np.float64) / NL.astype(np.float64) \
                + (R * R).sum(axis=0).astype(np.float64) / (nbag - NL).astype(np.float64)
        score[~ok] = -1.0
        t = int(np.argmax(score))                                   # first maximum: the smaller t
        if best is None or score[t] > best[0]:                      # features ascend: a tie keeps the smaller
            best = (score[t], f, t, int(NL[t]))
    return None if best is None else best[1:]


def grow(b, y, C, mult, mtry, seed, q_tree, p):
    """One tree, breadth first.  Returns (feature, threshold, left, cls) lists; -1 marks a leaf's feature, threshold and left."""
    feat, thr, left, cls = [-1], [-1], [-1], [0]
    level = [(0, np.flatnonzero(mult > 0))]
    for depth in range(MAX_DEPTH + 1):
        nxt = []
        for node, rows in level:                                    # ascending node id
            w = mult[rows]
            tot = np.bincount(y[rows], weights=w, minlength=C).astype(np.int64)
            cls[node] = int(np.argmax(tot))
            if np.count_nonzero(tot) <= 1 or tot.sum() < 2 or depth == MAX_DEPTH:
                continue
            s = best_split(b[rows], y[rows], w, C, candidates(seed, q_tree + node * p, p, mtry))
            if s is None:
                continue
            feat[node], thr[node], left[node] = s[0], s[1], len(feat)
            go = b[rows, s[0]] <= s[1]
            nxt += [(len(feat), rows[go]), (len(feat) + 1, rows[~go])]
            feat += [-1, -1]; thr += [-1, -1]; left += [-1, -1]; cls += [0, 0]
        level = nxt
    return feat, thr, left, cls


def forest(train, test, ltr, C, ntree, mtry=None, seed=0):
    """dict(feature, threshold, left, leaf_class (ntree x 2n, -1 beyond n_nodes), n_nodes, lo, hi, votes, prob, predictions)."""
    train, test, y = np.asarray(train, np.float64), np.asarray(test, np.float64), np.asarray(ltr, np.int64)
    n, p = train.shape
    mtry = max(1, int(np.floor(np.sqrt(p)))) if mtry is None else mtry
    lo, hi = bin_edges(train)
    b, tb = bins(train, lo, hi), bins(test, lo, hi)
    out = {k: np.full((ntree, 2 * n), -1, np.int32) for k in ("feature", "threshold", "left", "leaf_class")}
    n_nodes = np.zeros(ntree, np.int32)
    votes = np.zeros((test.shape[0], C), np.int32)
    for t in range(ntree):
        pick = np.minimum(np.floor(splitmix64_uniform(seed, t * n, n) * n).astype(np.int64), n - 1)
        mult = np.bincount(pick, minlength=n)
        arrays = grow(b, y, C, mult, mtry, seed, ntree * n + t * 2 * n * p, p)
        n_nodes[t] = len(arrays[0])
        for key, a in zip(("feature", "threshold", "left", "leaf_class"), arrays):
            out[key][t, :n_nodes[t]] = a
        f, th, le, cl = (np.array(a) for a in arrays)
        node = np.zeros(test.shape[0], np.int64)
        for _ in range(MAX_DEPTH + 1):
            inner = f[node] >= 0
            go = tb[np.arange(len(node)), np.maximum(f[node], 0)] <= th[node]
            node = np.where(inner, le[node] + np.where(go, 0, 1), node)
        np.add.at(votes, (np.arange(len(node)), cl[node]), 1)
    out.update(n_nodes=n_nodes, lo=lo, hi=hi, votes=votes, prob=votes / float(ntree), predictions=np.argmax(votes, axis=1))
    return out
