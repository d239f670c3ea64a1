"""numpy / pure-Python restatement of the embedding assessment (rcppml_gpu_assess; semantics of the reference's
src/gpu_bridge_assess.cu:358-753, restated in DESIGN.md section 4.8).

  MT19937           std::mt19937 (the C++ standard's engine: 10 000th output of the default seed 5489 is 4123659995)
  shuffle           libstdc++ 11's std::shuffle (bits/stl_algo.h): the two-positions-per-draw branch when (2^32-1) / n >= n, else
                    one draw per position, both through uniform_int_distribution's Lemire downscaling (_S_nd)
  kmeans_init / sil_plan / fold_plan   the random plan of the three seeded metrics
  ari / nmi         the contingency-table formulas, in the reference's summation order
  knn               exact top-k by (d, index); fp32 distances as an fmaf chain, emulated in float64 (exact whenever every product
                    and partial sum is exact in fp32, e.g. small integer coordinates)
  silhouette / classify / batch_mixing / kmeans   the metrics themselves
"""
import numpy as np

BIG = np.float32(1e30)
U32 = 0xFFFFFFFF


class MT19937:
    def __init__(self, seed=5489):
        self.mt = [0] * 624
        self.mt[0] = seed & U32
        for i in range(1, 624):
            self.mt[i] = (1812433253 * (self.mt[i - 1] ^ (self.mt[i - 1] >> 30)) + i) & U32
        self.idx = 624

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            v = mt[(i + 397) % 624] ^ (y >> 1)
            if y & 1:
                v ^= 0x9908B0DF
            mt[i] = v
        self.idx = 0

    def __call__(self):
        if self.idx >= 624:
            self._twist()
        y = self.mt[self.idx]
        self.idx += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y & U32


def _uniform(g, a, b):
    """uniform_int_distribution<unsigned long>{a, b}(g) with a 32-bit engine: Lemire's nearly-divisionless downscaling."""
    rng = b - a + 1                          # <= 2^32 - 1 on every path shuffle takes here
    prod = g() * rng
    low = prod & U32
    if low < rng:
        thr = ((1 << 32) - rng) % rng
        while low < thr:
            prod = g() * rng
            low = prod & U32
    return a + (prod >> 32)


def shuffle(seq, g):
    """In-place libstdc++ 11 std::shuffle of a list."""
    n = len(seq)
    if n == 0:
        return seq
    if U32 // n >= n:
        i = 1
        if n % 2 == 0:
            j = _uniform(g, 0, 1)
            seq[i], seq[j] = seq[j], seq[i]
            i += 1
        while i != n:
            r = i + 1
            x = _uniform(g, 0, r * (r + 1) - 1)
            p1, p2 = x // (r + 1), x % (r + 1)
            seq[i], seq[p1] = seq[p1], seq[i]
            i += 1
            seq[i], seq[p2] = seq[p2], seq[i]
            i += 1
        return seq
    for i in range(1, n):
        j = _uniform(g, 0, i)
        seq[i], seq[j] = seq[j], seq[i]
    return seq


def _seed(seed, off):
    return (int(seed) + off) & U32


def kmeans_init(n, K, nstart, seed):
    out = np.zeros((max(nstart, 0), K), np.int64)
    for r in range(nstart):
        idx = shuffle(list(range(n)), MT19937(_seed(seed, r)))
        out[r] = [idx[c % n] for c in range(K)]
    return out


def sil_plan(labels, n_classes, spc, seed):
    g = MT19937(_seed(seed, 100))
    samples, counts = [], []
    for c in range(n_classes):
        idx = [int(i) for i in np.flatnonzero(np.asarray(labels) == c)]
        counts.append(min(spc, len(idx)))
        shuffle(idx, g)
        samples.extend(idx[:max(counts[-1], 0)])
    return np.array(samples, np.int64), np.array(counts, np.int64)


def fold_plan(labels, n_classes, folds, seed):
    g = MT19937(_seed(seed, 200))
    labels = np.asarray(labels)
    fold = np.zeros(labels.shape[0], np.int64)
    for c in range(n_classes):
        idx = [int(i) for i in np.flatnonzero(labels == c)]
        shuffle(idx, g)
        for p, i in enumerate(idx):
            fold[i] = p % folds
    return fold


def _table(a, b):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    na, nb = max(int(a.max()), 0) + 1, max(int(b.max()), 0) + 1
    ct = np.zeros((na, nb), np.int64)
    np.add.at(ct, (a, b), 1)
    return ct


def ari(a, b):
    ct = _table(a, b)
    n = int(ct.sum())
    c2 = lambda x: x * (x - 1) / 2.0
    sij = 0.0
    for v in ct.ravel():
        sij += c2(int(v))
    si = 0.0
    for v in ct.sum(axis=1):
        si += c2(int(v))
    sj = 0.0
    for v in ct.sum(axis=0):
        sj += c2(int(v))
    cn = c2(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = np.float64(si) * sj / cn
        den = 0.5 * (si + sj) - expected
        return 0.0 if den == 0.0 else float((sij - expected) / den)


def nmi(a, b):
    import math
    ct = _table(a, b)
    n = int(ct.sum())
    na, nb = ct.shape
    pi, pj = [0.0] * na, [0.0] * nb
    for i in range(na):
        for j in range(nb):
            v = int(ct[i, j]) / n
            pi[i] += v
            pj[j] += v
    ha = hb = mi = 0.0
    for p in pi:
        if p > 0:
            ha -= p * math.log(p)
    for p in pj:
        if p > 0:
            hb -= p * math.log(p)
    for i in range(na):
        for j in range(nb):
            p = int(ct[i, j]) / n
            if p > 0 and pi[i] > 0 and pj[j] > 0:
                mi += p * math.log(p / (pi[i] * pj[j]))
    den = math.sqrt(ha * hb)
    return 0.0 if den == 0.0 else mi / den


def dist2(Q, C):
    """fp32 fmaf-chain squared distances (nq x nc), emulated in float64 with one fp32 rounding per step."""
    Q = np.asarray(Q, np.float32)
    C = np.asarray(C, np.float32)
    d = np.zeros((Q.shape[0], C.shape[0]), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(Q.shape[1]):
            df = (Q[:, j:j + 1] - C[None, :, j]).astype(np.float64)
            d = (df * df + d.astype(np.float64)).astype(np.float32)
    return d


def knn(Q, C=None, k=15, mask="none", group=None, group_k=None):
    """Exact top-k by (d, index) of candidates with d < 1e30 (NaN never chosen).  Returns idx (nq x k, -1 empty), dist (1e30 empty)."""
    self_ = C is None
    C = Q if self_ else C
    D = dist2(Q, C)
    nq, nc = D.shape
    idx = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), BIG, np.float32)
    cand = np.arange(nc)
    for q in range(nq):
        kq = k if (mask != "group" or group_k is None) else int(group_k[group[q]])
        ok = D[q] < BIG
        if mask == "self":
            ok &= cand != q
        elif mask == "group":
            ok &= np.asarray(group) != group[q]
        c = cand[ok]
        order = np.lexsort((c, D[q, c]))[:kq]
        idx[q, :len(order)] = c[order]
        dist[q, :len(order)] = D[q, c[order]]
    return idx, dist


def silhouette(X, labels, n_classes, spc, seed):
    """Per-point fp32 silhouette values and their double mean."""
    X = np.asarray(X, np.float32)
    labels = np.asarray(labels)
    n = X.shape[0]
    samples, counts = sil_plan(labels, n_classes, spc, seed)
    if spc < 0:
        s = np.full(n, np.float32(0.0 if n_classes >= 2 else 1.0), np.float32)
        return s, float(np.sum(s.astype(np.float64)))
    a = np.zeros(n, np.float32)
    b = np.full(n, BIG, np.float32)
    off = 0
    for c in range(n_classes):
        cnt = int(counts[c])
        if cnt <= 0:
            continue
        S = X[samples[off:off + cnt]]
        off += cnt
        sq = np.sqrt(np.maximum(dist2(X, S), np.float32(0)))
        tot = np.cumsum(sq, axis=1, dtype=np.float32)[:, -1]
        mean = (tot / np.float32(cnt)).astype(np.float32)
        own = labels == c
        a[own] = mean[own]
        other = ~own & (mean < b)
        b[other] = mean[other]
    den = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(den > 0, (b - a) / np.where(den > 0, den, 1), np.float32(0)).astype(np.float32)
    mean = 0.0
    for v in s:
        mean += float(v)
    return s, mean / n


def classify(X, labels, n_classes, k, folds, seed):
    """dict(fold_ids, fold_accuracy, fold_f1 (NaN: invalid fold), accuracy, f1, idx (the neighbour lists))."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    fid = fold_plan(labels, n_classes, folds, seed)
    ntest = np.bincount(fid, minlength=folds)
    kf = np.array([min(k, n - t) if (n - t > 0 and t > 0) else 0 for t in ntest])
    kmax = int(kf.max()) if kf.size else 0
    idx = knn(X, None, max(kmax, 1), mask="group", group=fid, group_k=kf)[0] if kmax > 0 else np.full((n, 1), -1)
    facc, ff1 = np.full(folds, np.nan), np.full(folds, np.nan)
    tacc = tf1 = 0.0
    valid = 0
    for f in range(folds):
        if not (n - ntest[f] > 0 and ntest[f] > 0):
            continue
        tp, fp, fn = np.zeros(n_classes, int), np.zeros(n_classes, int), np.zeros(n_classes, int)
        correct = 0
        for i in np.flatnonzero(fid == f):
            votes = np.zeros(n_classes, int)
            for j in idx[i, :kf[f]]:
                if j >= 0:
                    votes[labels[j]] += 1
            pred, truth = int(np.argmax(votes)), int(labels[i])
            if pred == truth:
                correct += 1
                tp[truth] += 1
            else:
                fp[pred] += 1
                fn[truth] += 1
        acc = correct / ntest[f]
        f1s = 0.0
        for c in range(n_classes):
            prec = tp[c] / (tp[c] + fp[c]) if tp[c] + fp[c] > 0 else 0
            rec = tp[c] / (tp[c] + fn[c]) if tp[c] + fn[c] > 0 else 0
            f1s += 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0
        f1 = f1s / max(n_classes, 1)
        facc[f], ff1[f] = acc, f1
        tacc += acc
        tf1 += f1
        valid += 1
    return dict(fold_ids=fid, fold_accuracy=facc, fold_f1=ff1, accuracy=tacc / valid if valid else 0.0,
                f1=tf1 / valid if valid else 0.0, idx=idx)


def batch_mixing(X, batch, n_batch, k):
    """Per-point normalised entropy and kNN silhouette, and their means (dict)."""
    import math
    batch = np.asarray(batch)
    n = batch.shape[0]
    kk = min(k, n - 1)
    if kk > 0:
        idx, dist = knn(X, None, kk, mask="self")
    else:
        idx, dist = np.full((n, 0), -1), np.zeros((n, 0), np.float32)
    hmax = math.log(n_batch)
    ent_pt, sil_pt = np.zeros(n), np.zeros(n)
    es = ss = 0.0
    for i in range(n):
        votes = np.zeros(n_batch, int)
        a = b = 0.0
        ac = bc = cnt = 0
        for e in range(kk):
            j = idx[i, e]
            if j < 0:
                continue
            votes[batch[j]] += 1
            d = float(np.sqrt(np.maximum(dist[i, e], np.float32(0))))
            if batch[j] == batch[i]:
                a += d
                ac += 1
            else:
                b += d
                bc += 1
            cnt += 1
        ent = 0.0
        for v in votes:
            if v > 0:
                p = v / cnt
                ent -= p * math.log(p)
        e_ = ent / hmax if hmax > 0 else 0.0
        ai = a / ac if ac > 0 else 0.0
        bi = b / bc if bc > 0 else ai
        den = max(ai, bi)
        s_ = (bi - ai) / den if den > 0 else 0.0
        ent_pt[i], sil_pt[i] = e_, s_
        es += e_
        ss += s_
    return dict(entropy_point=ent_pt, sil_point=sil_pt, entropy=es / n, sil=ss / n, idx=idx, dist=dist)


def kmeans(X, K, maxiter, seed, restart=0):
    """One restart: fp32 centroids from fp64 sums (rounded, then divided in fp32).  Returns (assignments of the last assign step,
    the smallest relative gap between the best and second-best centroid distance over all points and iterations)."""
    X = np.asarray(X, np.float32)
    n, dim = X.shape
    init = kmeans_init(n, K, restart + 1, seed)[restart]
    C = X[init].copy()
    gap = np.inf
    asg = np.zeros(n, np.int64)
    for _ in range(maxiter):
        D = ((X[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(-1)
        asg = np.argmin(D, axis=1)
        if K > 1:
            part = np.partition(D, 1, axis=1)
            gap = min(gap, float(np.min((part[:, 1] - part[:, 0]) / np.maximum(part[:, 1], 1e-300))))
        S = np.zeros((K, dim))
        np.add.at(S, asg, X.astype(np.float64))
        cnt = np.bincount(asg, minlength=K)
        C = (S.astype(np.float32) / np.maximum(cnt, 1).astype(np.float32)[:, None]).astype(np.float32)
    return asg, gap
