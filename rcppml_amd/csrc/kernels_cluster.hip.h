// kernels_cluster.hip.h -- the level-batched rank-2 ALS of bipartition() / dclust() (driver: ops_cluster.hip).
//
// A tree level holds C clusters.  Cluster c owns the level columns [seg[c], seg[c+1]) (its samples, gathered out of A in their
// order) and its own factors: W_c (2 x m, planes [c][0][*] and [c][1][*]) and h (2 x its columns, planes of the level's h).
// The level CSC (lp, li, lx) has one column per level column; its transpose (tp, ti, tx; stable, so within a row the level columns
// ascend) is cut into RUNS: maximal stretches of one row whose columns belong to one cluster.  A run is what A_S h needs for one
// (row, cluster) pair, so the W right-hand side is a plain segmented sum -- no atomics, fixed order, bitwise reproducible.
//
// Every reduction has a fixed order: a wavefront's lanes stride and fold by a shuffle tree, a workgroup's waves fold through LDS in
// wave order.  Per-cluster state (CL_* doubles, CI_* ints) lives in two small arrays; a cluster whose CI_ACTIVE flag is 0 is frozen
// and every kernel skips it, so each cluster stops at exactly the iteration its own convergence test ends it.
#pragma once
#include "common.hip.h"
#include "scan.hip.h"

namespace rcl {

constexpr int CL_STRIDE = 12;
enum { CL_AW00 = 0, CL_AW01, CL_AW11, CL_AH00, CL_AH01, CL_AH11, CL_D0, CL_D1, CL_TOL, CL_DIST, CL_N1, CL_N2 };
constexpr int CI_STRIDE = 4;
enum { CI_ACTIVE = 0, CI_ITER, CI_SIZE1, CI_SPARE };
constexpr int WG = 256;                  // one workgroup = 4 wavefronts
constexpr double TINY = 1e-15;           // reference core/constants.hpp tiny_num<double>()

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                            // lane 0 holds the sum
}
template <int G>
__device__ __forceinline__ double group_sum(double v) {           // sum over aligned groups of G lanes; the group's first lane holds it
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, G);
    return v;
}
// workgroup sum of NV values per thread, fixed order: lanes by shuffle tree, then waves 0..3; every thread receives the sums
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh /* 4 * NV */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double s = wave_sum(v[q]);
        if (lane == 0) sh[w * NV + q] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = ((sh[q] + sh[NV + q]) + sh[2 * NV + q]) + sh[3 * NV + q];
    __syncthreads();
}

// std::max(0.0, x) of nnls2 (bipartition.hpp:209-211): 0.0 unless 0.0 < x, so NaN becomes 0 (fmax would keep the other operand too,
// but differs for -0.0 / NaN in the first position; this is the comparison form)
__device__ __forceinline__ double cmax0(double x) { return 0.0 < x ? x : 0.0; }
__device__ __forceinline__ void solve2(const double* a /* a00 a01 a11 */, double b0, double b1, int nonneg, double& x0, double& x1) {
    const double denom = a[0] * a[2] - a[1] * a[1];
    x0 = (b0 * a[2] - b1 * a[1]) / denom;
    x1 = (b1 * a[0] - b0 * a[1]) / denom;
    if (nonneg) { x0 = cmax0(x0); x1 = cmax0(x1); }
}

// ----------------------------------------------------------------------------------------------------------------- level setup
// level column j of cluster c: col_of[j] = perm[poff[c] + j - seg[c]], clu_of[j] = c, cnt[j] = nonzeros of that column of A
__global__ __launch_bounds__(WG) void level_cols_kernel(const int* __restrict__ seg, const int* __restrict__ poff, const int* __restrict__ perm,
                                                        const int* __restrict__ Ap, int* __restrict__ col_of, int* __restrict__ clu_of,
                                                        int* __restrict__ cnt) {
    const int c = blockIdx.x;
    const int s0 = seg[c], s1 = seg[c + 1], po = poff[c];
    for (int j = s0 + (int)threadIdx.x; j < s1; j += WG) {
        const int col = perm[po + (j - s0)];
        col_of[j] = col; clu_of[j] = c;
        cnt[j] = Ap[col + 1] - Ap[col];
    }
}
// wave per level column: copy A's column col_of[j] into the level CSC
__global__ __launch_bounds__(WG) void level_gather_kernel(const int* __restrict__ Ap, const int* __restrict__ Ai, const double* __restrict__ Ax,
                                                          const int* __restrict__ col_of, const int* __restrict__ lp, int ncols,
                                                          int* __restrict__ li, double* __restrict__ lx) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= ncols) return;
    const int col = col_of[j], a0 = Ap[col], len = Ap[col + 1] - a0, o = lp[j];
    for (int e = lane; e < len; e += 64) { li[o + e] = Ai[a0 + e]; lx[o + e] = Ax[a0 + e]; }
}
// runs of the level CSR: rcnt[r] = number of runs of row r
__global__ __launch_bounds__(WG) void run_count_kernel(const int* __restrict__ tp, const int* __restrict__ ti, const int* __restrict__ clu_of,
                                                       int rows, int* __restrict__ rcnt) {
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r >= rows) return;
    int n = 0, prev = -1;
    for (int e = tp[r]; e < tp[r + 1]; ++e) {
        const int c = clu_of[ti[e]];
        n += c != prev;
        prev = c;
    }
    rcnt[r] = n;
}
__global__ __launch_bounds__(WG) void run_fill_kernel(const int* __restrict__ tp, const int* __restrict__ ti, const int* __restrict__ clu_of,
                                                      int rows, const int* __restrict__ roff, int* __restrict__ rstart, int* __restrict__ rrow,
                                                      int* __restrict__ rclu, int nruns, int nnz) {
    const int r = blockIdx.x * WG + threadIdx.x;
    if (r == 0) rstart[nruns] = nnz;
    if (r >= rows) return;
    int q = roff[r], prev = -1;
    for (int e = tp[r]; e < tp[r + 1]; ++e) {
        const int c = clu_of[ti[e]];
        if (c != prev) { rstart[q] = e; rrow[q] = r; rclu[q] = c; ++q; }
        prev = c;
    }
}
// every cluster starts from the same W (SplitMix64 draws, uploaded once) and its Gram; CI state reset
__global__ __launch_bounds__(WG) void init_kernel(const double* __restrict__ w0, int m, double* __restrict__ W, double* __restrict__ Wb,
                                                  double* __restrict__ cl, int* __restrict__ ci) {
    __shared__ double sh[4 * 3];
    const int c = blockIdx.x;
    double* Wc = W + (size_t)c * 2 * m;
    double* Bc = Wb + (size_t)c * 2 * m;
    double g[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < m; i += WG) {
        const double x0 = w0[i], x1 = w0[m + i];
        Wc[i] = x0; Wc[m + i] = x1; Bc[i] = 0; Bc[m + i] = 0;
        g[0] += x0 * x0; g[1] += x0 * x1; g[2] += x1 * x1;
    }
    block_sum<3>(g, sh);
    if (threadIdx.x == 0) {
        double* q = cl + (size_t)c * CL_STRIDE;
        q[CL_AW00] = g[0]; q[CL_AW01] = g[1]; q[CL_AW11] = g[2];
        q[CL_D0] = 1; q[CL_D1] = 1; q[CL_TOL] = 1; q[CL_DIST] = -1;
        int* s = ci + (size_t)c * CI_STRIDE;
        s[CI_ACTIVE] = 1; s[CI_ITER] = 0; s[CI_SIZE1] = 0; s[CI_SPARE] = 0;
    }
}

// ----------------------------------------------------------------------------------------------------------------- one ALS iteration
// H update (bipartition.hpp:251-264): wave per level column, b = W_c A_j in registers, closed-form 2 x 2 solve
__global__ __launch_bounds__(WG) void h_update_kernel(const int* __restrict__ lp, const int* __restrict__ li, const double* __restrict__ lx,
                                                      const int* __restrict__ clu_of, int ncols, int m, const double* __restrict__ W,
                                                      const double* __restrict__ cl, const int* __restrict__ ci, int nonneg,
                                                      double* __restrict__ h) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= ncols) return;
    const int c = clu_of[j];
    if (!ci[(size_t)c * CI_STRIDE + CI_ACTIVE]) return;
    const double* W0 = W + (size_t)c * 2 * m;
    const double* W1 = W0 + m;
    double b0 = 0, b1 = 0;
    for (int e = lp[j] + lane; e < lp[j + 1]; e += 64) {
        const int r = li[e];
        const double v = lx[e];
        b0 += v * W0[r]; b1 += v * W1[r];
    }
    b0 = wave_sum(b0); b1 = wave_sum(b1);
    if (lane == 0) {
        double x0, x1;
        solve2(cl + (size_t)c * CL_STRIDE + CL_AW00, b0, b1, nonneg, x0, x1);
        h[j] = x0; h[ncols + j] = x1;
    }
}
// scale(d, h) and a = h h^T (bipartition.hpp:265-268): workgroup per cluster
__global__ __launch_bounds__(WG) void h_scale_kernel(const int* __restrict__ seg, int ncols, double* __restrict__ h, double* __restrict__ cl,
                                                     const int* __restrict__ ci) {
    __shared__ double sh[4 * 3];
    const int c = blockIdx.x;
    if (!ci[(size_t)c * CI_STRIDE + CI_ACTIVE]) return;
    const int s0 = seg[c], s1 = seg[c + 1];
    double d[2] = {0, 0};
    for (int j = s0 + (int)threadIdx.x; j < s1; j += WG) { d[0] += h[j]; d[1] += h[ncols + j]; }
    block_sum<2>(d, sh);
    d[0] += TINY; d[1] += TINY;
    double g[3] = {0, 0, 0};
    for (int j = s0 + (int)threadIdx.x; j < s1; j += WG) {
        const double x0 = h[j] / d[0], x1 = h[ncols + j] / d[1];
        h[j] = x0; h[ncols + j] = x1;
        g[0] += x0 * x0; g[1] += x0 * x1; g[2] += x1 * x1;
    }
    block_sum<3>(g, sh);
    if (threadIdx.x == 0) {
        double* q = cl + (size_t)c * CL_STRIDE;
        q[CL_AH00] = g[0]; q[CL_AH01] = g[1]; q[CL_AH11] = g[2];
    }
}
// W right-hand side (bipartition.hpp:272-279): G lanes per run, Wb[c][*][row] = sum over the run of A_rj h_j
template <int G>
__global__ __launch_bounds__(WG) void w_rhs_kernel(const int* __restrict__ rstart, const int* __restrict__ rrow, const int* __restrict__ rclu,
                                                   int nruns, const int* __restrict__ ti, const double* __restrict__ tx, const double* __restrict__ h,
                                                   int ncols, int m, const int* __restrict__ ci, double* __restrict__ Wb) {
    const int gid = blockIdx.x * (WG / G) + threadIdx.x / G, sub = threadIdx.x & (G - 1);
    if (gid >= nruns) return;                           // whole groups leave together: the group shuffle below sees only live lanes
    const int c = rclu[gid];
    if (!ci[(size_t)c * CI_STRIDE + CI_ACTIVE]) return;
    double b0 = 0, b1 = 0;
    for (int e = rstart[gid] + sub; e < rstart[gid + 1]; e += G) {
        const int j = ti[e];
        const double v = tx[e];
        b0 += v * h[j]; b1 += v * h[ncols + j];
    }
    b0 = group_sum<G>(b0); b1 = group_sum<G>(b1);
    if (sub == 0) {
        double* B = Wb + (size_t)c * 2 * m;
        B[rrow[gid]] = b0; B[m + rrow[gid]] = b1;
    }
}
// nnls2InPlace + scale(d, w) + cor(w, w_it) + the next a = w w^T (bipartition.hpp:280-284), workgroup per cluster.  The solve runs
// on every row (rows without a nonzero in the subset solve b = 0, as on the CPU).  Wb is zeroed behind the read, ready for the
// next iteration.  The convergence test freezes the cluster: CI_ACTIVE = (iter < maxit && tol_ > tol) -- NaN tol_ stops it.
__global__ __launch_bounds__(WG) void w_finish_kernel(int m, double* __restrict__ W, double* __restrict__ Wb, double* __restrict__ cl,
                                                      int* __restrict__ ci, int nonneg, int maxit, double tol, int* __restrict__ any_active) {
    __shared__ double sh[4 * 8];
    const int c = blockIdx.x;
    int* s = ci + (size_t)c * CI_STRIDE;
    if (!s[CI_ACTIVE]) return;
    double* q = cl + (size_t)c * CL_STRIDE;
    const double a[3] = {q[CL_AH00], q[CL_AH01], q[CL_AH11]};
    double* Wc = W + (size_t)c * 2 * m;
    double* Bc = Wb + (size_t)c * 2 * m;
    double d[2] = {0, 0};
    for (int i = threadIdx.x; i < m; i += WG) {
        double x0, x1;
        solve2(a, Bc[i], Bc[m + i], nonneg, x0, x1);
        d[0] += x0; d[1] += x1;
    }
    block_sum<2>(d, sh);
    d[0] += TINY; d[1] += TINY;
    // sums: x.y, x, y, x.x, y.y (x = previous w, y = new w) and the new Gram
    double r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < m; i += WG) {
        double x0, x1;
        solve2(a, Bc[i], Bc[m + i], nonneg, x0, x1);
        Bc[i] = 0; Bc[m + i] = 0;
        const double y0 = x0 / d[0], y1 = x1 / d[1];
        const double p0 = Wc[i], p1 = Wc[m + i];
        Wc[i] = y0; Wc[m + i] = y1;
        r[0] += p0 * y0 + p1 * y1;
        r[1] += p0 + p1;
        r[2] += y0 + y1;
        r[3] += p0 * p0 + p1 * p1;
        r[4] += y0 * y0 + y1 * y1;
        r[5] += y0 * y0; r[6] += y0 * y1; r[7] += y1 * y1;
    }
    block_sum<8>(r, sh);
    if (threadIdx.x == 0) {
        const double n = 2.0 * (double)m;
        const double num = n * r[0] - r[1] * r[2];
        const double den = sqrt((n * r[3] - r[1] * r[1]) * (n * r[4] - r[2] * r[2]));
        const double tol_ = 1.0 - num / den;
        q[CL_D0] = d[0]; q[CL_D1] = d[1]; q[CL_TOL] = tol_;
        q[CL_AW00] = r[5]; q[CL_AW01] = r[6]; q[CL_AW11] = r[7];
        const int it = s[CI_ITER] + 1;
        s[CI_ITER] = it;
        const int on = (it < maxit && tol_ > tol) ? 1 : 0;
        s[CI_ACTIVE] = on;
        if (on) *any_active = 1;          // a plain store of 1 by every cluster still running: no read-modify-write
    }
}

// ----------------------------------------------------------------------------------------------------------------- after convergence
// v by the orientation of d (bipartition.hpp:291-303); side[j] = 1 for samples1 (v > 0; zero and NaN go to samples2)
__global__ __launch_bounds__(WG) void orient_kernel(const int* __restrict__ clu_of, int ncols, const double* __restrict__ h,
                                                    const double* __restrict__ cl, double* __restrict__ v, int* __restrict__ side) {
    const int j = blockIdx.x * WG + threadIdx.x;
    if (j >= ncols) return;
    const double* q = cl + (size_t)clu_of[j] * CL_STRIDE;
    const double x = q[CL_D0] > q[CL_D1] ? h[j] - h[ncols + j] : h[ncols + j] - h[j];
    v[j] = x;
    side[j] = x > 0 ? 1 : 0;
}
// stable partition of each segment (workgroup per cluster, a scan over 256-column tiles): samples1 first, then samples2, both in
// their order, written back over the cluster's stretch of perm (col_of holds the level's copy of it)
__global__ __launch_bounds__(WG) void partition_kernel(const int* __restrict__ seg, const int* __restrict__ poff, const int* __restrict__ col_of,
                                                       const int* __restrict__ side, int* __restrict__ perm, int* __restrict__ ci) {
    __shared__ int sh[4];
    const int c = blockIdx.x;
    const int s0 = seg[c], s1 = seg[c + 1], po = poff[c];
    int n1 = 0;
    for (int j = s0 + (int)threadIdx.x; j < s1; j += WG) n1 += side[j];
    for (int off = 32; off > 0; off >>= 1) n1 += __shfl_down(n1, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = n1;
    __syncthreads();
    const int size1 = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    int run1 = 0, run2 = 0;                    // how many of each side the tiles before this one held
    for (int t = s0; t < s1; t += WG) {
        const int j = t + (int)threadIdx.x;
        const int f = j < s1 ? side[j] : 0;
        int tot1;
        const int ex1 = rk::scan_block_excl(f, sh, &tot1);
        const int ex2 = (int)threadIdx.x - ex1;          // side-0 columns before this one in the tile
        if (j < s1) perm[po + (f ? run1 + ex1 : size1 + run2 + ex2)] = col_of[j];
        run1 += tot1;
        run2 += min(WG, s1 - t) - tot1;
    }
    if (threadIdx.x == 0) ci[(size_t)c * CI_STRIDE + CI_SIZE1] = size1;
}
// centroid sums by runs (the W-pass shape with an indicator in place of h): Wb[c][0][row] = sum of the run's values on side 1,
// Wb[c][1][row] on side 0.  side == nullptr (leaves): everything into plane 0.
template <int G>
__global__ __launch_bounds__(WG) void centroid_rows_kernel(const int* __restrict__ rstart, const int* __restrict__ rrow, const int* __restrict__ rclu,
                                                           int nruns, const int* __restrict__ ti, const double* __restrict__ tx,
                                                           const int* __restrict__ side, int m, int planes, double* __restrict__ Wb) {
    const int gid = blockIdx.x * (WG / G) + threadIdx.x / G, sub = threadIdx.x & (G - 1);
    if (gid >= nruns) return;
    const int c = rclu[gid];
    double s1 = 0, s2 = 0;
    for (int e = rstart[gid] + sub; e < rstart[gid + 1]; e += G) {
        const double v = tx[e];
        if (!side || side[ti[e]]) s1 += v; else s2 += v;
    }
    s1 = group_sum<G>(s1); s2 = group_sum<G>(s2);
    if (sub == 0) {
        double* B = Wb + (size_t)c * planes * m;
        B[rrow[gid]] = s1;
        if (planes == 2) B[m + rrow[gid]] = s2;
    }
}
// centers of both children (centroid(): `/= size`, bipartition.hpp:46-48) into W, their norms into CL_N1 / CL_N2; Wb zeroed
__global__ __launch_bounds__(WG) void center_finish_kernel(const int* __restrict__ seg, int m, double* __restrict__ W, double* __restrict__ Wb,
                                                           double* __restrict__ cl, const int* __restrict__ ci) {
    __shared__ double sh[4 * 2];
    const int c = blockIdx.x;
    const double n1 = (double)ci[(size_t)c * CI_STRIDE + CI_SIZE1];
    const double n2 = (double)(seg[c + 1] - seg[c]) - n1;
    double* Wc = W + (size_t)c * 2 * m;
    double* Bc = Wb + (size_t)c * 2 * m;
    double r[2] = {0, 0};
    for (int i = threadIdx.x; i < m; i += WG) {
        const double c1 = Bc[i] / n1, c2 = Bc[m + i] / n2;
        Bc[i] = 0; Bc[m + i] = 0;
        Wc[i] = c1; Wc[m + i] = c2;
        r[0] += c1 * c1; r[1] += c2 * c2;
    }
    block_sum<2>(r, sh);
    if (threadIdx.x == 0) { cl[(size_t)c * CL_STRIDE + CL_N1] = sqrt(r[0]); cl[(size_t)c * CL_STRIDE + CL_N2] = sqrt(r[1]); }
}
// rel_cosine terms (bipartition.hpp:93-126), wave per level column: side 1: sqrt(x.c2) |c1| / (sqrt(x.c1) |c2|), side 0 mirrored
__global__ __launch_bounds__(WG) void relcos_kernel(const int* __restrict__ lp, const int* __restrict__ li, const double* __restrict__ lx,
                                                    const int* __restrict__ clu_of, const int* __restrict__ side, int ncols, int m,
                                                    const double* __restrict__ W, const double* __restrict__ cl, double* __restrict__ term) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= ncols) return;
    const int c = clu_of[j];
    const double* C1 = W + (size_t)c * 2 * m;
    const double* C2 = C1 + m;
    double x1 = 0, x2 = 0;
    for (int e = lp[j] + lane; e < lp[j + 1]; e += 64) {
        const int r = li[e];
        const double v = lx[e];
        x1 += C1[r] * v; x2 += C2[r] * v;
    }
    x1 = wave_sum(x1); x2 = wave_sum(x2);
    if (lane == 0) {
        const double* q = cl + (size_t)c * CL_STRIDE;
        term[j] = side[j] ? (sqrt(x2) * q[CL_N1]) / (sqrt(x1) * q[CL_N2]) : (sqrt(x1) * q[CL_N2]) / (sqrt(x2) * q[CL_N1]);
    }
}
__global__ __launch_bounds__(WG) void dist_finish_kernel(const int* __restrict__ seg, const int* __restrict__ side, const double* __restrict__ term,
                                                         int m, double* __restrict__ cl) {
    __shared__ double sh[4 * 2];
    const int c = blockIdx.x;
    double r[2] = {0, 0};
    for (int j = seg[c] + (int)threadIdx.x; j < seg[c + 1]; j += WG) {
        if (side[j]) r[0] += term[j]; else r[1] += term[j];
    }
    block_sum<2>(r, sh);
    if (threadIdx.x == 0) cl[(size_t)c * CL_STRIDE + CL_DIST] = (r[0] + r[1]) / (2.0 * (double)m);
}
// leaf centers (compute_centroid(): `*= 1 / size`, bipartition.hpp:68-90) from plane-0 sums, into out (C x m)
__global__ __launch_bounds__(WG) void leaf_center_kernel(const int* __restrict__ seg, int m, const double* __restrict__ sums,
                                                         double* __restrict__ out) {
    const int c = blockIdx.x;
    const double inv = 1.0 / (double)(seg[c + 1] - seg[c]);
    for (int i = threadIdx.x; i < m; i += WG) out[(size_t)c * m + i] = sums[(size_t)c * m + i] * inv;
}

}  // namespace rcl
