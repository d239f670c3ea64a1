// knn_launch.hip.h -- the launcher of the exact fp32 top-k (knn_partial / knn_merge, kernels_assess.hip.h), defined in
// ops_assess.hip and shared with ops_classify.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace rcppml_plugin {

// dQ nq x dim, dC nc x dim (device, fp32).  mode 0 none, 1 exclude the query's own index, 2 exclude the query's group (dgroup; dgk,
// may be null: k per group).  d_oi / d_od: nq x kmax, the k smallest candidates in (distance, index) order, -1 / 1e30 when empty.
// Synchronises the stream before it returns.
void knn_device(const float* dQ, int nq, const float* dC, int nc, int dim, int mode, const int* dgroup, const int* dgk, int k, int kmax,
                int* d_oi, float* d_od, hipStream_t s);

}  // namespace rcppml_plugin
