// ops_dense.hip -- dense-input right-hand sides of the ALS update (device-level C ABI, include/rcppml_gpu.h layer 2).
// Reference: primitives::rhs<CPU> on a dense A (B = W_T * A, Eigen GEMM) and detail::rhs_transpose (B = H * A^T),
// nmf/fit_cpu.hpp:547-549 / :783; the reference's GPU build calls cuBLAS for them (nmf/fit_gpu_dense.cuh).
// Hand-written skinny MFMA GEMMs (kernels_dense.hip.h: fp32 on 32x32x2 tiles, fp64 on 16x16x4 tiles) that stream A once per
// product; no BLAS library is linked (tools/probe/dense_check.py times torch.matmul = rocBLAS/hipBLASLt beside them).  Everything around them (Gram, features,
// NNLS solve, scaling, loss) is the hand-written path shared with the sparse input.
#include "common.hip.h"
#include "kernels_dense.hip.h"
#include <cstring>


// Launch geometry of one product, from the problem size alone.  The output columns (n forward, m backward) are cut into blocks of
// `per_block`; the reduction (m forward, n backward) into chunks of DENSE_KC / DENSE_KC_BWD indices, split over `slices` grid rows
// of `rchunk` indices each (a multiple of the chunk; the last slice may be shorter) so that about 4096 / 4 blocks are in flight
// whatever the output width is.  slices == 1 writes B directly, otherwise per-slice partials are summed by dense_reduce.
// rcppml_hip_rhs_dense launches exactly this; rcppml_hip_rhs_dense_geometry reports it.
struct dense_rhs_geom {
    int64_t blocks, slices, rchunk;
    int rt;          // row-tile template parameter: fp32 k <= 32 rt (1..4), fp64 k <= 16 rt (1, 2, 4, 8)
};
static inline dense_rhs_geom dense_rhs_geometry(int dtype, int64_t m, int64_t n, int k, int transposed) {
    const bool f32 = dtype == RCPPML_F32;
    dense_rhs_geom g;
    if (f32) { g.rt = (k + 31) / 32; if (g.rt > 4) g.rt = 4; }
    else g.rt = k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 8;
    const int64_t out_cols = transposed ? m : n, red = transposed ? n : m;
    const int64_t per_block = f32 ? (transposed ? 512 : 128) : (transposed ? 128 : 64);
    const int64_t kc = transposed ? rk::DENSE_KC_BWD : rk::DENSE_KC;
    g.blocks = (out_cols + per_block - 1) / per_block;
    const int64_t chunks = (red + kc - 1) / kc;
    int64_t slices = (4096 + g.blocks * 4 - 1) / (g.blocks * 4);
    if (f32 && !transposed) {
        const char* es = exp_env("RCPPML_GPU_DENSE_SLICES");
        if (es) slices = atoi(es);
    }
    if (slices > chunks) slices = chunks;
    if (slices < 1) slices = 1;
    g.rchunk = (chunks + slices - 1) / slices * kc;
    g.slices = (red + g.rchunk - 1) / g.rchunk;
    return g;
}

static void dense_rhs_check(int64_t m, int64_t n, int k) {
    if (m > 0x7FFFFFFF || n > 0x7FFFFFFF) throw std::runtime_error("rhs_dense: dimension exceeds int32");
    if (k > 128) throw std::runtime_error("rhs_dense: k must be <= 128");
}

// out[0] = blocks (grid x), out[1] = slices (grid y), out[2] = reduction indices per slice, out[3] = row-tile template parameter;
// all zero for an empty problem (nothing is launched).  Host arithmetic only: no device is touched.
extern "C" int rcppml_hip_rhs_dense_geometry(int dtype, int64_t m, int64_t n, int k, int transposed, int64_t* out) {
    try {
        if (!out) throw std::runtime_error("rhs_dense_geometry: out is null");
        if (dtype != RCPPML_F32 && dtype != RCPPML_F64) throw std::runtime_error("rhs_dense_geometry: unknown dtype");
        out[0] = out[1] = out[2] = out[3] = 0;
        if (m <= 0 || n <= 0 || k <= 0) return 0;
        dense_rhs_check(m, n, k);
        const dense_rhs_geom g = dense_rhs_geometry(dtype, m, n, k, transposed);
        out[0] = g.blocks; out[1] = g.slices; out[2] = g.rchunk; out[3] = g.rt;
        return 0;
    }
    RCPPML_CATCH_RET
}

// transposed = 0:  B (k x n) = F (k x m) * A (m x n)       transposed = 1:  B (k x m) = F (k x n) * A^T
// A is column-major m x n; F and B are column-major with leading dimension k.
extern "C" int rcppml_hip_rhs_dense(rcppml_hip_ctx* c, int dtype, const void* A, int64_t m, int64_t n, int transposed,
                                    const void* F, int k, void* B) {
    try {
        HIPCHK(hipSetDevice(c->device));
        if (m <= 0 || n <= 0 || k <= 0) return 0;
        dense_rhs_check(m, n, k);
        const dense_rhs_geom g = dense_rhs_geometry(dtype, m, n, k, transposed);
        const int64_t slices = g.slices, out_cols = transposed ? m : n;
        const dim3 grid((unsigned)g.blocks, (unsigned)slices);
        const int64_t count = (int64_t)k * out_cols;
        if (dtype == RCPPML_F32) {
            const float* Af = (const float*)A; const float* Ff = (const float*)F; float* Bf = (float*)B;
            float* part = slices == 1 ? Bf : static_cast<float*>(c->scratch(WS_GRAPH, (size_t)slices * k * out_cols * sizeof(float)));
#define RCPPML_DENSE32(KERN)                                                                                                      \
            switch (g.rt) {                                                                                                       \
                case 1: hipLaunchKernelGGL((rk::KERN<1>), grid, dim3(256), 0, c->stream, Af, m, n, Ff, k, g.rchunk, part); break; \
                case 2: hipLaunchKernelGGL((rk::KERN<2>), grid, dim3(256), 0, c->stream, Af, m, n, Ff, k, g.rchunk, part); break; \
                case 3: hipLaunchKernelGGL((rk::KERN<3>), grid, dim3(256), 0, c->stream, Af, m, n, Ff, k, g.rchunk, part); break; \
                default: hipLaunchKernelGGL((rk::KERN<4>), grid, dim3(256), 0, c->stream, Af, m, n, Ff, k, g.rchunk, part); break; \
            }
            if (!transposed) { RCPPML_DENSE32(dense_rhs_fwd_f32) } else { RCPPML_DENSE32(dense_rhs_bwd_f32) }
#undef RCPPML_DENSE32
            if (slices > 1) {
                HIPCHK(hipGetLastError());
                hipLaunchKernelGGL(rk::dense_reduce_f32, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, part, count, (int)slices, Bf);
            }
            HIPCHK(hipGetLastError());
            return 0;
        }
        {
            const double* Ad = (const double*)A; const double* Fd = (const double*)F; double* Bd = (double*)B;
            double* part = slices == 1 ? Bd : static_cast<double*>(c->scratch(WS_GRAPH, (size_t)slices * k * out_cols * sizeof(double)));
#define RCPPML_DENSE64(KERN)                                                                                                      \
            switch (g.rt) {                                                                                                       \
                case 1: hipLaunchKernelGGL((rk::KERN<1>), grid, dim3(256), 0, c->stream, Ad, m, n, Fd, k, g.rchunk, part); break; \
                case 2: hipLaunchKernelGGL((rk::KERN<2>), grid, dim3(256), 0, c->stream, Ad, m, n, Fd, k, g.rchunk, part); break; \
                case 4: hipLaunchKernelGGL((rk::KERN<4>), grid, dim3(256), 0, c->stream, Ad, m, n, Fd, k, g.rchunk, part); break; \
                default: hipLaunchKernelGGL((rk::KERN<8>), grid, dim3(256), 0, c->stream, Ad, m, n, Fd, k, g.rchunk, part); break; \
            }
            if (!transposed) { RCPPML_DENSE64(dense_rhs_fwd_f64) } else { RCPPML_DENSE64(dense_rhs_bwd_f64) }
#undef RCPPML_DENSE64
            HIPCHK(hipGetLastError());
            if (slices > 1) {
                hipLaunchKernelGGL(rk::dense_reduce<double>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, c->stream, part, count, (int)slices, Bd);
                HIPCHK(hipGetLastError());
            }
            return 0;
        }
    }
    RCPPML_CATCH_RET
}
