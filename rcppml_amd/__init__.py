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
             path (csrc/ops_classify.hip); classify_rf(): the histogram random forest (csrc/ops_classify_rf.hip)
  similarity.py cosine() / bipartiteMatch() / align(): mirror of the R surface on the HIP similarity path (csrc/ops_similarity.hip):
             sparse column cosines (rcppml_gpu_cosine_sparse_ex, tile geometry from rcppml_gpu_cosine_geometry), batched dense
             cosines / correlations (rcppml_gpu_cosine_dense_ex) and the host assignment solver (rcppml_gpu_bipartite_match_ex).  A
             zero-norm column has similarity 0 to every column; two deviations from R (cosine(vector, matrix) returns the cosine,
             align() applies the inverse of the matching), see the module docstring; and, build-defined, cosine_knn() (the k best
             columns without the full matrix, rcppml_gpu_cosine_knn_sparse_ex) and knn_graph() (the graph Laplacian nmf(graph_H=) takes)
  factor_net.py factor_input() / nmf_layer() / svd_layer() / factor_shared() / factor_concat() / factor_add() / factor_condition() /
             factor_net() / fit() / predict(): mirror of the R factor-graph surface; multi-layer graphs run the reference's deep fit
             resident on the device (csrc/ops_graph.hip)
  streaming.py nmf_streaming(): the plain MSE fit with the matrix streamed through the device one column panel at a time
             (csrc/ops_stream.hip); neither the matrix nor its transpose is resident
  svd_streaming.py svd_streaming() / pca_streaming(): the randomized block SVD with the matrix streamed the same way
             (csrc/ops_stream_svd.hip), from a host CSC or an .spz path
  streampress.py st_write() / st_read() / st_info(): StreamPress v2 `.spz` files; st_write() encodes a host CSC on the device
             (csrc/ops_spz_write.hip: symbolise, histogram, normalise, rANS encode, escapes) into what the two streamed entries take
  als.py     one-process-per-GPU column-sharded ALS loop over torch.distributed (RCCL): Comm, ShardedALS, HipOps
  data.py    synthetic inputs (restatement of R/simulateNMF.R) and CSC helpers
"""
__version__ = "0.1.0"

# the package attribute `refine` is the function from here on; the module's other names come with `from rcppml_amd.refine import ...`
from .refine import compute_target, refine  # noqa: E402,F401
from .classify import classify_cv, classify_embedding, classify_logistic, classify_rf  # noqa: E402,F401
from .similarity import align, bipartiteMatch, cosine, cosine_knn, knn_graph  # noqa: E402,F401
from .streaming import nmf_streaming  # noqa: E402,F401
from .svd_streaming import pca_streaming, svd_streaming  # noqa: E402,F401
from .streampress import st_info, st_read, st_write  # noqa: E402,F401
