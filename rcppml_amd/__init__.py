"""rcppml_amd -- MI355X (gfx950) backend for RcppML's alternating-NNLS NMF hot path.

Layout (only what the path needs):
  csrc/      hand-written HIP kernels + the C-ABI (include/rcppml_gpu.h) -> lib/RcppML_gpu.so
  _abi.py    ctypes binding of that C-ABI (no CPU fallback: fails loudly if the library is missing)
  nmf.py     host-side mirror of the reference R surface: nmf() / nnls() / predict() / evaluate()
  cluster.py bipartition() / dclust(): mirror of the R surface on the HIP clustering path (csrc/ops_cluster.hip)
  svd.py     svd() / pca(): mirror of the R surface on the HIP truncated-SVD path (csrc/ops_svd.hip)
  assess.py  assess() / knn(): mirror of the R surface on the HIP embedding-assessment path (csrc/ops_assess.hip)
  distribution.py score_test_distribution() / diagnose_zero_inflation() / diagnose_dispersion() / auto_nmf_distribution(): mirror of
             the R surface on the HIP distribution-diagnostics path (csrc/ops_distribution.hip)
  consensus.py consensus_nmf() / consensus_matrix() / hclust_average(): mirror of the R surface on the HIP consensus-clustering
             path (csrc/ops_consensus.hip)
  refine.py  compute_target() / refine(): mirror of the R surface on the HIP label-guided refinement path (csrc/ops_refine.hip)
  zi.py      nmf_zi(): zero-inflated GP / NB NMF (zi = "row" / "col") on the HIP zero-inflation path (csrc/ops_zi.hip); nmf(zi = ...)
             itself still refuses, routing it here is a later change
  classify.py classify_embedding() / classify_logistic() / classify_cv(): mirror of the R surface on the HIP classifier-evaluation
             path (csrc/ops_classify.hip)
  similarity.py cosine() / bipartiteMatch() / align(): mirror of the R surface on the HIP similarity path (csrc/ops_similarity.hip):
             sparse column cosines (rcppml_gpu_cosine_sparse_ex, tile geometry from rcppml_gpu_cosine_geometry), batched dense
             cosines / correlations (rcppml_gpu_cosine_dense_ex) and the host assignment solver (rcppml_gpu_bipartite_match_ex).  A
             zero-norm column has similarity 0 to every column; two deviations from R (cosine(vector, matrix) returns the cosine,
             align() applies the inverse of the matching), see the module docstring
  factor_net.py factor_input() / nmf_layer() / svd_layer() / factor_shared() / factor_concat() / factor_add() / factor_condition() /
             factor_net() / fit() / predict(): mirror of the R factor-graph surface; multi-layer graphs run the reference's deep fit
             resident on the device (csrc/ops_graph.hip)
  als.py     one-process-per-GPU column-sharded ALS loop over torch.distributed (RCCL): Comm, ShardedALS, HipOps
  data.py    synthetic inputs (restatement of R/simulateNMF.R) and CSC helpers
"""
__version__ = "0.1.0"

# the package attribute `refine` is the function from here on; the module's other names come with `from rcppml_amd.refine import ...`
from .refine import compute_target, refine  # noqa: E402,F401
from .classify import classify_cv, classify_embedding, classify_logistic  # noqa: E402,F401
from .similarity import align, bipartiteMatch, cosine  # noqa: E402,F401
