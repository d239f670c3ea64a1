"""Consensus clustering: host-side mirror of the reference's consensus_nmf (R/consensus.R:75-158) on the HIP path
(csrc/ops_consensus.hip).  The replicates are fitted by nmf() one after another; the m x m consensus matrix is built on the device
from their stacked loadings (hard co-clustering counts, or the Jaccard overlap of cosine kNN sets), and the average-linkage tree,
its cut and the cophenetic correlation come from the library's host entry.  Where the reference leaves the answer open this build
has two rules: equal similarities go to the lower index, and a sample whose loading is all zero has similarity 0 to every sample.
Tree ties go to the pair with the smallest lower, then upper, index (believed to be R's hclust; not verified against R).  Plot and
summary methods and the streaming (file path) input are not provided.  No CPU fallback: without a device the consensus stage
raises BackendError."""
import numpy as np

from . import _abi
from . import nmf as _nmf
from ._abi import _check
from .distribution import match_arg

METHODS = ("hard", "knn_jaccard")


def consensus_matrix(W_list, method="hard", knn=10):
    """The consensus matrix (m x m) of fitted loadings: W_list holds reps arrays m x k (a model's `w`).  Returns dict(consensus,
    labels): labels is reps x m (0-based dominant factor per sample) for "hard", None for "knn_jaccard"."""
    method = match_arg(method, METHODS)
    Ws = [np.asarray(w, np.float64) for w in W_list]
    if not Ws or any(w.ndim != 2 or w.shape != Ws[0].shape for w in Ws):
        raise ValueError("W_list must hold at least one matrix, all m x k")
    m, k = Ws[0].shape
    r = _check(_abi.consensus_double(np.stack(Ws), m, k, len(Ws), method, knn), "consensus")
    return dict(consensus=r["consensus"], labels=r["labels"])


def hclust_average(dist, k):
    """hclust(as.dist(dist), "average") with cutree(k) and the cophenetic correlation: dict(merge ((m - 1) x 2, R's convention),
    height, clusters (1..k by first appearance), cophenetic).  Only dist[i, j] with i > j is read.  Runs on the host."""
    r = _check(_abi.hclust_average_double(np.asarray(dist, np.float64), k), "hclust")
    return dict(merge=r["merge"], height=r["height"], clusters=r["clusters"], cophenetic=r["cophenetic"])


def consensus_nmf(data, k, reps=50, method=METHODS, knn=10, seed=None, verbose=False, **nmf_kwargs):
    """R's consensus_nmf: `reps` fits nmf(data, k, seed=seed + i, verbose=False, ...) for i = 1..reps (seed=None passes None), the
    consensus matrix of their `w`, the average-linkage tree on 1 - consensus cut into k clusters, and the cophenetic correlation.
    Samples are the rows of `data`.  Returns dict(consensus, models, clusters, cophenetic, merge, height, k, reps, method, knn);
    knn is None for "hard"."""
    method = match_arg(method, METHODS)
    if isinstance(data, (str, bytes)):
        raise NotImplementedError("consensus_nmf on a file path (streaming input) is not implemented by the MI355X backend")
    reps = int(reps)
    if verbose:
        print("Running %d NMF replicates for consensus clustering (method: %s )..." % (reps, method))
    models = []
    for i in range(1, reps + 1):
        models.append(_nmf.nmf(data, k, seed=None if seed is None else seed + i, verbose=False, **nmf_kwargs))
    cons = consensus_matrix([mod.w for mod in models], method, knn)["consensus"]
    tree = hclust_average(1.0 - cons, k)
    if verbose:
        print("\nCophenetic correlation: %s (higher = more stable clustering)" % round(tree["cophenetic"], 4))
    return dict(consensus=cons, models=models, clusters=tree["clusters"], cophenetic=tree["cophenetic"], merge=tree["merge"],
                height=tree["height"], k=k, reps=reps, method=method, knn=knn if method == "knn_jaccard" else None)
