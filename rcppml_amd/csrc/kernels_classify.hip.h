// kernels_classify.hip.h -- device kernels of the classifier evaluation entries (ops_classify.hip).  fp64 throughout (the kNN
// distances themselves come from kernels_assess.hip.h, fp32), no floating-point atomics: every sum is taken in a fixed order over
// fixed row chunks, so the results do not depend on the grid and two runs are bitwise equal.
//
//   knn_vote                  one wave per test row: the k neighbour labels are tabulated into C integer counters (LDS), written
//                             out as counts / k; the prediction is the first maximum.
//   irls_pass / irls_solve    one-vs-rest binomial(logit) IRLS with R's glm.fit arithmetic, all C fits advancing together.
//                             irls_pass reads each 32-row tile of X = [1 | train] once into LDS and forms, for every class that is
//                             still running, eta / mu / the deviance terms from the previous beta and the weighted Gram and rhs
//                             partials of the next solve (fp64 VALU; the tile's products x_ri x_rj are shared by the 8 classes of a
//                             batch).  Partials are kept per 128-row chunk: a chunk's four tiles are added in tile order by the
//                             thread that owns the entry.  irls_solve (one workgroup per class) adds the chunk partials in chunk
//                             order, decides convergence of the previous solve on the device, and solves the normal equations by a
//                             right-looking Cholesky that skips (aliases) a column whose pivot is <= 1e-11 x the largest diagonal.
//   logit_predict             test probabilities, row-normalised, and the first maximum.
//   prob_argmax / confusion_count / auc_pairs   the metrics: integer counts only (64-bit pair counts for the AUC).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rcl {

constexpr int TILE = 32;               // rows of one LDS tile
constexpr int CHUNK = 128;             // rows of one partial sum (4 tiles); fixed, so the sums do not depend on the grid
constexpr int CB = 8;                  // classes per batch (share the tile's products)
constexpr int PMAX = 129;              // intercept + 128 columns
constexpr int THREADS = 256;
constexpr double kEps = 2.220446049250313e-16;     // DBL_EPSILON
constexpr double kPivotTol = 1e-11;

// first maximum of row[0 .. C) (R's which.max)
__device__ inline int first_max(const double* row, int C) {
    int best = 0;
    double bv = row[0];
    for (int c = 1; c < C; ++c)
        if (row[c] > bv) { bv = row[c]; best = c; }
    return best;
}

// ---------------------------------------------------------------------------------------------------------------- kNN votes
// nn: n_test x k train indices (all valid: k <= n_train).  Block = one wave, one test row.  LDS: C ints.
__global__ __launch_bounds__(64) void knn_vote(const int* __restrict__ nn, const int* __restrict__ train_labels, int n_test, int k,
                                               int C, double* __restrict__ votes, int* __restrict__ pred) {
    extern __shared__ int cnt[];
    const int i = blockIdx.x, lane = threadIdx.x;
    for (int c = lane; c < C; c += 64) cnt[c] = 0;
    __syncthreads();
    for (int e = lane; e < k; e += 64) {
        const int j = nn[(size_t)i * k + e];
        if (j >= 0) atomicAdd(&cnt[train_labels[j]], 1);          // integer counts: order-free
    }
    __syncthreads();
    double* v = votes + (size_t)i * C;
    for (int c = lane; c < C; c += 64) v[c] = (double)cnt[c] / (double)k;
    if (lane == 0) {
        int best = 0;
        for (int c = 1; c < C; ++c)
            if (cnt[c] > cnt[best]) best = c;
        pred[i] = best;
    }
}

// ---------------------------------------------------------------------------------------------------------------- IRLS
struct IrlsArgs {
    const double* X;          // n x p train rows (row-major, without the intercept)
    const int* y;             // n labels in [0, C)
    int n, p, P, C;           // P = p + 1
    int nchunk;               // ceil(n / CHUNK)
    double* beta;             // C x P
    double* Gp;               // nchunk x C x P x P (lower triangle used)
    double* bp;               // nchunk x C x P
    double* dp;               // nchunk x C deviance partials (sum of -log terms, without the factor 2)
    double* A;                // C x P x P workspace of the solve
    int* aliased;             // C x P
    int* done;                // C
    int* iters;               // C
    int* converged;           // C
    double* deviance;         // C
    double* devold;           // C
    int* ndone;               // 1: classes done
    int maxit;
    double epsilon;
};

// dynamic LDS of irls_pass, in doubles
__host__ __device__ inline size_t irls_pass_lds_doubles(int P) { return (size_t)TILE * P + (size_t)CB * P + 3 * (size_t)CB * TILE; }

// first != 0: the start mu = (y + 0.5) / 2 stands in for beta.  Any grid: block b takes chunks b, b + gridDim.x, ...
__global__ __launch_bounds__(THREADS) void irls_pass(IrlsArgs a, int first) {
    extern __shared__ double sm[];
    const int P = a.P, p = a.p, C = a.C, tid = threadIdx.x;
    double* xs = sm;                            // TILE x P
    double* bs = xs + (size_t)TILE * P;         // CB x P
    double* sw = bs + (size_t)CB * P;           // CB x TILE weights
    double* swz = sw + CB * TILE;               // CB x TILE weight * working response
    double* sdv = swz + CB * TILE;              // CB x TILE deviance terms
    for (int chunk = blockIdx.x; chunk < a.nchunk; chunk += gridDim.x) {
        const int r0c = chunk * CHUNK;
        const int ntile = (min(a.n, r0c + CHUNK) - r0c + TILE - 1) / TILE;
        for (int t = 0; t < ntile; ++t) {
            const int r0 = r0c + t * TILE;
            __syncthreads();
            for (int e = tid; e < TILE * P; e += THREADS) {
                const int r = e / P, j = e % P, row = r0 + r;
                xs[e] = row < a.n ? (j == 0 ? 1.0 : a.X[(size_t)row * p + (j - 1)]) : 0.0;
            }
            for (int c0 = 0; c0 < C; c0 += CB) {
                __syncthreads();
                if (!first)
                    for (int e = tid; e < CB * P; e += THREADS) {
                        const int c = c0 + e / P;
                        bs[e] = c < C ? a.beta[(size_t)c * P + e % P] : 0.0;
                    }
                __syncthreads();
                {   // phase A: thread (r, cb) -> eta, mu, deviance term, weight, working response of row r for class c0 + cb
                    const int r = tid & (TILE - 1), cb = tid / TILE, c = c0 + cb, row = r0 + r;
                    double w = 0.0, wz = 0.0, dv = 0.0;
                    if (c < C && row < a.n && !a.done[c]) {
                        const double y = a.y[row] == c ? 1.0 : 0.0;
                        double eta, mu;
                        if (first) {
                            mu = (y + 0.5) / 2.0;
                            eta = log(mu / (1.0 - mu));
                        } else {
                            eta = 0.0;
                            const double* xr = xs + (size_t)r * P;
                            const double* b = bs + (size_t)cb * P;
                            for (int j = 0; j < P; ++j) eta = __builtin_fma(xr[j], b[j], eta);
                            const double tt = eta < -30.0 ? kEps : (eta > 30.0 ? 1.0 / kEps : exp(eta));
                            mu = tt / (1.0 + tt);
                        }
                        const double om = 1.0 - mu;
                        dv = y == 1.0 ? -log(mu) : -log(om);
                        const double ae = fabs(eta);
                        double g = kEps;
                        if (!(ae > 30.0)) {
                            const double ex = exp(-ae), op = 1.0 + ex;
                            g = fmax(ex / (op * op), kEps);
                        }
                        const double z = eta + (y - mu) / g;
                        w = g * g / (mu * om);
                        wz = w * z;
                    }
                    sw[cb * TILE + r] = w; swz[cb * TILE + r] = wz; sdv[cb * TILE + r] = dv;
                }
                __syncthreads();
                // phase B: the lower triangle of the weighted Gram, rows in order; x_ri x_rj is shared by the batch's classes
                for (int e = tid; e < P * P; e += THREADS) {
                    const int i = e / P, j = e % P;
                    if (j > i) continue;
                    double acc[CB];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) acc[cb] = 0.0;
                    for (int r = 0; r < TILE; ++r) {
                        const double pr = xs[(size_t)r * P + i] * xs[(size_t)r * P + j];
#pragma unroll
                        for (int cb = 0; cb < CB; ++cb) acc[cb] = __builtin_fma(sw[cb * TILE + r], pr, acc[cb]);
                    }
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) {
                        const int c = c0 + cb;
                        if (c >= C || a.done[c]) continue;
                        double* g = a.Gp + ((size_t)chunk * C + c) * P * P + e;
                        *g = t == 0 ? acc[cb] : *g + acc[cb];
                    }
                }
                for (int e = tid; e < CB * P; e += THREADS) {          // rhs
                    const int cb = e / P, i = e % P, c = c0 + cb;
                    if (c >= C || a.done[c]) continue;
                    double s = 0.0;
                    for (int r = 0; r < TILE; ++r) s = __builtin_fma(swz[cb * TILE + r], xs[(size_t)r * P + i], s);
                    double* g = a.bp + ((size_t)chunk * C + c) * P + i;
                    *g = t == 0 ? s : *g + s;
                }
                if (tid < CB) {                                          // deviance terms, rows in order
                    const int c = c0 + tid;
                    if (c < C && !a.done[c]) {
                        double s = 0.0;
                        for (int r = 0; r < TILE; ++r) s += sdv[tid * TILE + r];
                        double* g = a.dp + (size_t)chunk * C + c;
                        *g = t == 0 ? s : *g + s;
                    }
                }
            }
        }
    }
}

// Launch L = 1, 2, ..., maxit + 1, after the L-th irls_pass.  The deviance that pass formed belongs to solve L - 1 (L = 1: the start
// values): a class converges when |dev - devold| / (|dev| + 0.1) < epsilon, and is frozen with iters = L - 1.  Otherwise solve L is
// made, unless L > maxit (iters = maxit, not converged).  Grid = C, block = THREADS.
__global__ __launch_bounds__(THREADS) void irls_solve(IrlsArgs a, int L) {
    __shared__ double sb[PMAX], sd[PMAX];
    __shared__ int sal[PMAX];
    __shared__ double s_maxdiag;
    __shared__ int s_stop;
    const int c = blockIdx.x, tid = threadIdx.x, P = a.P, C = a.C;
    if (a.done[c]) return;
    if (tid == 0) {
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += a.dp[(size_t)ch * C + c];
        const double dev = 2.0 * s;
        int stop = 0;
        a.deviance[c] = dev;
        if (L > 1 && fabs(dev - a.devold[c]) / (fabs(dev) + 0.1) < a.epsilon) {
            a.converged[c] = 1;
            stop = 1;
        } else if (L > a.maxit) {
            stop = 1;
        }
        a.devold[c] = dev;
        if (stop) {
            a.iters[c] = L - 1;
            a.done[c] = 1;
            atomicAdd(a.ndone, 1);
        }
        s_stop = stop;
    }
    __syncthreads();
    if (s_stop) return;
    double* A = a.A + (size_t)c * P * P;
    for (int e = tid; e < P * P; e += THREADS) {
        if (e % P > e / P) continue;
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += a.Gp[((size_t)ch * C + c) * P * P + e];
        A[e] = s;
    }
    for (int i = tid; i < P; i += THREADS) {
        double s = 0.0;
        for (int ch = 0; ch < a.nchunk; ++ch) s += a.bp[((size_t)ch * C + c) * P + i];
        sb[i] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double m = 0.0;
        for (int i = 0; i < P; ++i) m = fmax(m, A[(size_t)i * P + i]);
        s_maxdiag = m;
    }
    __syncthreads();
    const double floor_ = kPivotTol * s_maxdiag;
    // right-looking Cholesky on the lower triangle; an aliased column is skipped as a pivot, as a row and as a column
    for (int j = 0; j < P; ++j) {
        const double piv = A[(size_t)j * P + j];
        const bool al = !(piv > floor_);
        if (tid == 0) { sal[j] = al; sd[j] = al ? 1.0 : sqrt(piv); }
        if (al) continue;
        const double ljj = sqrt(piv);
        for (int i = j + 1 + tid; i < P; i += THREADS) A[(size_t)i * P + j] /= ljj;
        __syncthreads();
        const int m = P - 1 - j;
        for (int q = tid; q < m * m; q += THREADS) {
            const int i = j + 1 + q / m, k = j + 1 + q % m;
            if (k <= i) A[(size_t)i * P + k] -= A[(size_t)i * P + j] * A[(size_t)k * P + j];
        }
        __syncthreads();
    }
    __syncthreads();
    for (int j = 0; j < P; ++j) {                      // L y = b
        if (sal[j]) continue;
        const double yj = sb[j] / sd[j];
        __syncthreads();
        if (tid == 0) sb[j] = yj;
        for (int i = j + 1 + tid; i < P; i += THREADS)
            if (!sal[i]) sb[i] -= A[(size_t)i * P + j] * yj;
        __syncthreads();
    }
    for (int j = P - 1; j >= 0; --j) {                 // L' beta = y
        if (sal[j]) continue;
        const double xj = sb[j] / sd[j];
        __syncthreads();
        if (tid == 0) sb[j] = xj;
        for (int i = tid; i < j; i += THREADS)
            if (!sal[i]) sb[i] -= A[(size_t)j * P + i] * xj;
        __syncthreads();
    }
    for (int j = tid; j < P; j += THREADS) {
        a.beta[(size_t)c * P + j] = sal[j] ? 0.0 : sb[j];
        a.aliased[(size_t)c * P + j] = sal[j];
    }
}

// One thread per test row: mu_c = linkinv(x . beta_c), divided by the row sum (0 -> 1), and the first maximum.
__global__ __launch_bounds__(THREADS) void logit_predict(const double* __restrict__ T, int n_test, int p, const double* __restrict__ beta,
                                                         int C, double* __restrict__ prob, int* __restrict__ pred) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_test) return;
    const int P = p + 1;
    const double* x = T + (size_t)i * p;
    double* pr = prob + (size_t)i * C;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const double* b = beta + (size_t)c * P;
        double eta = b[0];                                   // fma(1, b0, 0)
        for (int j = 0; j < p; ++j) eta = __builtin_fma(x[j], b[j + 1], eta);
        const double tt = eta < -30.0 ? kEps : (eta > 30.0 ? 1.0 / kEps : exp(eta));
        const double mu = tt / (1.0 + tt);
        pr[c] = mu;
        sum += mu;
    }
    if (sum == 0.0) sum = 1.0;
    for (int c = 0; c < C; ++c) pr[c] = pr[c] / sum;
    pred[i] = first_max(pr, C);
}

// ---------------------------------------------------------------------------------------------------------------- metrics
__global__ __launch_bounds__(THREADS) void prob_argmax(const double* __restrict__ prob, int n_test, int C, int* __restrict__ pred) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_test) pred[i] = first_max(prob + (size_t)i * C, C);
}

// conf (C x C, zeroed): rows true, columns predicted.  Integer atomics: order-free.
__global__ __launch_bounds__(THREADS) void confusion_count(const int* __restrict__ truth, const int* __restrict__ pred, int n_test, int C,
                                                           int* __restrict__ conf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_test) atomicAdd(&conf[(size_t)truth[i] * C + pred[i]], 1);
}

// R's .compute_auc counts, under a stable descending sort, the pairs (positive i, negative j) with i before j: s_i > s_j, or
// s_i == s_j and i < j.  Grid (ceil(n_test / THREADS), C): thread = one j of class blockIdx.y's one-vs-rest problem; the positives
// pass through LDS a tile at a time.  out[c * gridDim.x + block]: 64-bit pair counts (the host adds them in block order).
__global__ __launch_bounds__(THREADS) void auc_pairs(const double* __restrict__ prob, const int* __restrict__ truth, int n_test, int C,
                                                     unsigned long long* __restrict__ out) {
    __shared__ double ss[THREADS];
    __shared__ int sp[THREADS];
    __shared__ unsigned long long red[THREADS];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int j = blockIdx.x * THREADS + tid;
    const bool neg = j < n_test && truth[j] != c;
    const double sj = j < n_test ? prob[(size_t)j * C + c] : 0.0;
    unsigned long long cnt = 0;
    for (int i0 = 0; i0 < n_test; i0 += THREADS) {
        const int i = i0 + tid;
        __syncthreads();
        ss[tid] = i < n_test ? prob[(size_t)i * C + c] : 0.0;
        sp[tid] = i < n_test && truth[i] == c;
        __syncthreads();
        if (neg) {
            const int lim = min(THREADS, n_test - i0);
            for (int q = 0; q < lim; ++q)
                if (sp[q] && (ss[q] > sj || (ss[q] == sj && i0 + q < j))) ++cnt;
        }
    }
    red[tid] = cnt;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[(size_t)c * gridDim.x + blockIdx.x] = red[0];
}

}  // namespace rcl
