"""Plain numpy restatement of consensus clustering as the reference's consensus_nmf computes it on the CPU (R/consensus.R:102-137,
src/RcppFunctions_utils.cpp:560-618), written from the description of its semantics; the tests compare the HIP path and the
library's host tree with it.

hard:        label = first maximum of each row of W_r (which.max), connectivity[i, j] = replicates with equal labels, / reps.
knn_jaccard: per replicate, rows scaled to unit 2-norm, sim = Wn Wn^T, actual_k = min(knn, m - 1), the neighbour set of i = the
             actual_k largest sim[i, j] with j != i, J = |Si & Sj| / (2 actual_k - |Si & Sj|) (0 when the denominator is 0), diagonal
             1; connectivity += J in replicate order, then / reps.  Two rules where the reference is undefined: equal similarities go
             to the lower index, and a zero-norm row has similarity 0 to every sample.
tree:        average linkage on the entries below the diagonal; each step merges the smallest dissimilarity, among equal minima the
             smallest lower index, then the smallest upper index; the merged cluster keeps the lower slot, Lance-Williams
             (na da + nb db) / (na + nb).  merge in R's convention, clusters numbered by first appearance, Pearson cophenetic
             correlation with a two-pass mean, NaN when either side is constant.
"""
import numpy as np


def labels(W):
    """which.max per row, 0-based (np.argmax returns the first maximum)."""
    return np.argmax(np.asarray(W, np.float64), axis=1).astype(np.int32)


def hard(W_list):
    """(consensus, labels reps x m)."""
    L = np.stack([labels(W) for W in W_list])
    reps, m = L.shape
    conn = np.zeros((m, m), np.float64)
    for r in range(reps):
        conn += (L[r][:, None] == L[r][None, :])
    return conn / reps, L


def similarity(W, blas=False):
    """Cosine similarity of the rows: squares added in column order, W / sqrt(sum), products added in column order (so that equal
    rows give exactly equal similarities, which a blocked matrix product does not promise).  blas=True forms Wn Wn^T with the
    library product instead: faster, the same to rounding, for inputs without exact ties."""
    W = np.asarray(W, np.float64)
    m, k = W.shape
    s = np.zeros(m)
    for f in range(k):
        s = s + W[:, f] * W[:, f]
    nrm = np.sqrt(s)
    Wn = np.where(nrm[:, None] > 0, W / np.where(nrm > 0, nrm, 1.0)[:, None], 0.0)
    if blas:
        return Wn @ Wn.T
    sim = np.zeros((m, m))
    for f in range(k):
        sim += np.outer(Wn[:, f], Wn[:, f])
    return sim


def knn_sets(sim, knn):
    """(member m x m bool, margin m): member[i, j] = j in the neighbour set of i; margin[i] = sim of the actual_k-th neighbour minus
    the next candidate's (inf when every other sample is a neighbour)."""
    m = sim.shape[0]
    K = min(int(knn), m - 1)
    s = sim.copy()
    np.fill_diagonal(s, -np.inf)                       # self is no candidate
    if K < m - 1:                                      # ascending positions of the K-th and (K + 1)-th largest
        part = np.partition(s, (m - K - 1, m - K), axis=1)
        thr = part[:, m - K]
        margin = thr - part[:, m - K - 1]
    else:
        thr = np.partition(s, m - K, axis=1)[:, m - K]
        margin = np.full(m, np.inf)
    above = s > thr[:, None]
    equal = s == thr[:, None]
    need = K - above.sum(1)
    member = above | (equal & (np.cumsum(equal, axis=1) <= need[:, None]))      # equal values: the lower indices first
    assert (member.sum(1) == K).all() and not member.diagonal().any()
    return member, margin


def intersections(member):
    """|Si & Sj| for all pairs (integer sparse products), through whichever of the sets or their complements is sparser."""
    import scipy.sparse as sp
    m = member.shape[0]
    if 2 * int(member.sum()) <= member.size:
        B = sp.csr_matrix(member.astype(np.int64))
        return np.asarray((B @ B.T).todense())
    C = sp.csr_matrix((~member).astype(np.int64))      # |Si & Sj| = m - |Ci| - |Cj| + |Ci & Cj|
    n = (~member).sum(1).astype(np.int64)
    return m - n[:, None] - n[None, :] + np.asarray((C @ C.T).todense())


def jaccard(W, knn, blas=False):
    """(J, margin, member) of one replicate."""
    sim = similarity(W, blas)
    member, margin = knn_sets(sim, knn)
    m = sim.shape[0]
    K = min(int(knn), m - 1)
    inter = intersections(member)
    union = 2 * K - inter
    J = np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)
    np.fill_diagonal(J, 1.0)
    return J, margin, member


def knn_jaccard(W_list, knn, blas=False):
    """(consensus, margins reps x m, members list of m x m bool)."""
    conn = None
    margins, members = [], []
    for W in W_list:
        J, mg, mem = jaccard(W, knn, blas)
        conn = np.zeros_like(J) if conn is None else conn
        conn += J
        margins.append(mg)
        members.append(mem)
    return conn / len(W_list), np.stack(margins), members


def consensus(W_list, method, knn=10):
    return hard(W_list)[0] if method == "hard" else knn_jaccard(W_list, knn)[0]


def hclust_average(dist, k_cut):
    """Naive O(m^3) tree: dict(merge, height, clusters, cophenetic, sets (the sample sets merged at each step))."""
    dist = np.asarray(dist, np.float64)
    m = dist.shape[0]
    D = np.full((m, m), np.inf)
    il = np.tril_indices(m, -1)
    D[il[1], il[0]] = dist[il]                         # D[lower index, upper index]
    active = list(range(m))
    size = [1] * m
    name = [-(i + 1) for i in range(m)]
    sets = [[i] for i in range(m)]
    merge = np.zeros((m - 1, 2), np.int32)
    height = np.zeros(m - 1)
    coph = np.zeros((m, m))
    steps = []
    for s in range(m - 1):
        best = None
        for a in active:                               # ascending lower index, then ascending upper index; strict <
            for b in active:
                if b > a and (best is None or D[a, b] < best[0]):
                    best = (D[a, b], a, b)
        h, a, b = best
        na, nb = name[a], name[b]
        if na < 0 and nb < 0:
            pair = (na, nb)                            # both samples: a < b, the lower sample first
        elif na > 0 and nb > 0:
            pair = (min(na, nb), max(na, nb))
        else:
            pair = (min(na, nb), max(na, nb))          # the sample (negative) first
        merge[s] = pair
        height[s] = h
        steps.append((list(sets[a]), list(sets[b])))
        for u in sets[a]:
            for v in sets[b]:
                coph[max(u, v), min(u, v)] = h
        for c in active:
            if c != a and c != b:
                dac = D[min(a, c), max(a, c)]
                dbc = D[min(b, c), max(b, c)]
                D[min(a, c), max(a, c)] = (size[a] * dac + size[b] * dbc) / (size[a] + size[b])
        sets[a] = sets[a] + sets[b]
        size[a] += size[b]
        name[a] = s + 1
        active.remove(b)
    # cutree: the first m - k_cut merges, clusters numbered by first appearance
    root = list(range(m))
    for s in range(m - k_cut):
        sa, sb = steps[s]
        for v in sb:
            root[v] = root[sa[0]]
    number, clusters = {}, np.zeros(m, np.int32)
    for i in range(m):
        clusters[i] = number.setdefault(root[i], len(number) + 1)
    x, y = dist[il], coph[il]
    if x.min() == x.max() or y.min() == y.max():
        cor = float("nan")
    else:
        dx, dy = x - x.mean(), y - y.mean()
        cor = float(np.clip((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum()), -1.0, 1.0))
    return dict(merge=merge, height=height, clusters=clusters, cophenetic=cor, sets=steps)
