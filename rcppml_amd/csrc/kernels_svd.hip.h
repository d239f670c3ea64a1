// kernels_svd.hip.h -- device kernels of the truncated SVD / PCA entries (ops_svd.hip).
//
// Two matrix-vector products and a family of elementwise kernels that end in fixed-order block partial sums:
//   spmv_t  y = A' x   one wavefront per column (CSC gather, or a column of the column-major dense matrix)
//   spmv    y = A x    one wavefront per row of the CSR (the device transpose of the CSC), or one thread per dense row
// Every reduction is two-stage: a block writes the partial sums of its CH-element chunk (one wavefront per column, a butterfly
// shuffle), and each consumer re-adds the partials of all blocks in block order.  No float atomics: two runs are bitwise equal.
//
// Per-factor / per-step freezing without host synchronisation: kernels of iteration `it` run only while it < st[S_STOP].  A kernel
// that ends the loop in iteration `it` writes st[S_STOP] = it + 1, so the other workgroups of that same kernel (and the rest of
// iteration `it`) still run, and every later launch of the factor is an early-exiting no-op.
#pragma once
#include <hip/hip_runtime.h>

namespace rsv {

constexpr int WG = 256, WAVE = 64, NW = WG / WAVE;
constexpr int PER = 8, CH = WG * PER;          // elements per block of the elementwise kernels
constexpr int NPMAX = 4096;                    // partial columns a consumer finalises into LDS

// state words (int): first iteration that does not run, break in the v-update, break in the u-update, iterations / steps done
enum { S_STOP = 0, S_BRKV = 2, S_BRKU = 3, S_ITERS = 4, S_WORDS = 8 };

template <class T> __device__ inline T wave_sum(T v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The columns a chunk of x is dotted with: nx columns of X (leading dimension ld), then ne extra vectors -- a vector, nullptr for
// all-ones (a plain sum), or the global x itself (its squared norm).
template <class T> struct Cols {
    const T* X = nullptr; long ld = 0; int nx = 0;
    const T* e[3] = {nullptr, nullptr, nullptr}; int ne = 0;
    __host__ __device__ int np() const { return nx + ne; }
};

// partials of the chunk xs (LDS, rows r0 .. r0 + cnt of the global vector xg) against C -> P[blockIdx.x * np + c]
template <class T> __device__ void block_partials(const T* xs, const T* xg, long r0, int cnt, const Cols<T>& C, T* P) {
    const int w = threadIdx.x / WAVE, l = threadIdx.x % WAVE, np = C.np();
    for (int c = w; c < np; c += NW) {
        const T* col = c < C.nx ? C.X + (long)c * C.ld : C.e[c - C.nx];
        const bool self = c >= C.nx && col == xg;
        T acc = 0;
        for (int r = l; r < cnt; r += WAVE) acc += (self ? xs[r] : col ? col[r0 + r] : T(1)) * xs[r];
        acc = wave_sum(acc);
        if (l == 0) P[(long)blockIdx.x * np + c] = acc;
    }
}

// h[c] = sum over blocks b = 0 .. nb-1 of P[b * np + c], in block order (every consumer block gets the same bits)
template <class T> __device__ void finalize(const T* P, int nb, int np, T* h) {
    for (int c = threadIdx.x; c < np; c += WG) {
        T s = 0;
        for (int b = 0; b < nb; ++b) s += P[(long)b * np + c];
        h[c] = s;
    }
    __syncthreads();
}

// deflation.hpp:192-236: L2 shrink, L1 soft threshold, nonneg, upper bound
template <class T> __device__ inline T regularize(T x, T l1, T l2, int nonneg, T ub, T nsq) {
    if (l2 > 0) x *= T(1) / (T(1) + l2 / nsq);
    if (l1 > 0) {
        const T th = l1 / (T(2) * nsq);
        x = x > th ? x - th : (x < -th ? x + th : T(0));
    }
    if (nonneg) x = x > T(0) ? x : T(0);
    if (ub > 0) x = x < ub ? x : ub;
    return x;
}

__device__ inline bool idle(const int* st, int it) { return st && it >= st[S_STOP]; }

// ------------------------------------------------------------------------------------------------------------ products
template <class T>
__global__ __launch_bounds__(WG) void spmv_t_csc(const int* __restrict__ p, const int* __restrict__ ri, const T* __restrict__ x,
                                                 int n, const T* __restrict__ u, T* __restrict__ y, const int* st, int it, int brk) {
    if (idle(st, it) || (brk && st[brk])) return;
    const int j = blockIdx.x * NW + threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    if (j >= n) return;
    T acc = 0;
    for (int e = p[j] + l; e < p[j + 1]; e += WAVE) acc += x[e] * u[ri[e]];
    acc = wave_sum(acc);
    if (l == 0) y[j] = acc;
}
template <class T>
__global__ __launch_bounds__(WG) void spmv_t_dense(const T* __restrict__ A, int m, int n, const T* __restrict__ u, T* __restrict__ y,
                                                   const int* st, int it, int brk) {
    if (idle(st, it) || (brk && st[brk])) return;
    const int j = blockIdx.x * NW + threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    if (j >= n) return;
    const T* a = A + (long)j * m;
    T acc = 0;
    for (int i = l; i < m; i += WAVE) acc += a[i] * u[i];
    acc = wave_sum(acc);
    if (l == 0) y[j] = acc;
}
// rows of A from the CSR (tp / tj / tx: the CSC of A^T)
template <class T>
__global__ __launch_bounds__(WG) void spmv_csr(const int* __restrict__ tp, const int* __restrict__ tj, const T* __restrict__ tx,
                                               int m, const T* __restrict__ v, T* __restrict__ y, const int* st, int it, int brk) {
    if (idle(st, it) || (brk && st[brk])) return;
    const int i = blockIdx.x * NW + threadIdx.x / WAVE, l = threadIdx.x % WAVE;
    if (i >= m) return;
    T acc = 0;
    for (int e = tp[i] + l; e < tp[i + 1]; e += WAVE) acc += tx[e] * v[tj[e]];
    acc = wave_sum(acc);
    if (l == 0) y[i] = acc;
}
// A thread adds the n terms of its row one after the other.  In float that serial sum drifts by about sqrt(n) eps, where the
// other three products split a sum over 64 lanes first: at n = 6145 the fp32 dense fit sat 15 times further from the float64
// restatement than the restatement's own float32 run (4 times is the suite's bound), the CSC fit of the same shape 1.5 times.  So
// the float row is summed in double (the products are exact there) and rounded once; the double row is summed as before.  The
// kernel is bound by its one read of A, not by these adds.
template <class T> struct RowSum { using type = T; };
template <> struct RowSum<float> { using type = double; };
template <class T>
__global__ __launch_bounds__(WG) void spmv_dense(const T* __restrict__ A, int m, int n, const T* __restrict__ v, T* __restrict__ y,
                                                 const int* st, int it, int brk) {
    if (idle(st, it) || (brk && st[brk])) return;
    const int i = blockIdx.x * WG + threadIdx.x;
    if (i >= m) return;
    using S = typename RowSum<T>::type;
    S acc = 0;
    for (int j = 0; j < n; ++j) acc += (S)A[(long)j * m + i] * (S)v[j];
    y[i] = (T)acc;
}

// ------------------------------------------------------------------------------------------------------------ partials
// P = partials of x (len) against C
template <class T>
__global__ __launch_bounds__(WG) void dots_kernel(const T* __restrict__ x, long len, Cols<T> C, T* __restrict__ P) {
    __shared__ T xs[CH];
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) xs[r] = x[r0 + r];
    __syncthreads();
    block_partials(xs, x, r0, cnt, C, P);
}

// ------------------------------------------------------------------------------------------------------------ deflation
enum { M_LOOP = 0, M_WARM = 1, M_PLAIN = 2 };

// v-update epilogue (n): h = finalised m-side partials [U_k' u_hat (k), mu . u_hat, |u_hat|^2];
//   s = y - center * (mu . u_hat) - V_k diag(d) (U_k' u_hat);  LOOP: v = regularize(s / (dc |u_hat|^2));  WARM: v = s.
// dc: the cross-validation denominator correction (deflation.hpp:552-559, :724-739), 1 without CV; it scales |u_hat|^2 where it
// divides the update and where regularize() takes it, and nowhere else.
// Writes vraw and the n-side partials [V_k' v (k), sum v, |v|^2].
template <class T>
__global__ __launch_bounds__(WG) void defl_v_kernel(const T* __restrict__ y, int n, const T* __restrict__ V, int k,
                                                    const T* __restrict__ d, const T* __restrict__ Pm, int nbm, int center, T l1, T l2,
                                                    int nonneg, T ub, T dc, int mode, T* __restrict__ vraw, T* __restrict__ Pn, int* st,
                                                    int it) {
    if (idle(st, it)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    finalize(Pm, nbm, k + 2, h);
    const T c = center ? h[k] : T(0), usq = h[k + 1] * dc;
    const bool brk = mode == M_LOOP && !(usq > T(0));
    if (brk && blockIdx.x == 0 && threadIdx.x == 0) st[S_BRKV] = 1;
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)n - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long j = r0 + r;
        T s = y[j] - c;
        for (int q = 0; q < k; ++q) s -= V[(long)q * n + j] * (d[q] * h[q]);
        if (mode == M_LOOP) s = brk ? T(0) : regularize(s / usq, l1, l2, nonneg, ub, usq);
        xs[r] = s;
        vraw[j] = s;
    }
    __syncthreads();
    Cols<T> C;
    C.X = V; C.ld = n; C.nx = k; C.e[0] = nullptr; C.e[1] = vraw; C.ne = 2;
    block_partials(xs, vraw, r0, cnt, C, Pn);
}

// u-update epilogue (m): hv = finalised n-side partials [V_k' vraw, sum vraw, |vraw|^2], sv = |vraw|.
//   LOOP / WARM: v = vraw / sv (grid-stride over n); t = t / sv - center * mu * sum / sv - U_k diag(d) (V_k' vraw) / sv
//   PLAIN (Rayleigh quotient): t - center * mu * sum - U_k diag(d) (V_k' v), nothing normalised.
//   LOOP: u_raw = regularize(t / (dc |v|^2)), dc as in defl_v_kernel.  Writes u_raw and the partials [|u_raw|^2, u_raw . u_cur].
template <class T>
__global__ __launch_bounds__(WG) void defl_u_kernel(const T* __restrict__ t, int m, const T* __restrict__ U, int k,
                                                    const T* __restrict__ d, const T* __restrict__ Pn, int nbn, const T* __restrict__ mu,
                                                    T l1, T l2, int nonneg, T ub, T dc, int mode, const T* __restrict__ vraw,
                                                    T* __restrict__ v, int n, T* __restrict__ uraw, const T* __restrict__ ucur,
                                                    T* __restrict__ Pu, int* st, int it) {
    if (idle(st, it)) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    const bool loop = mode == M_LOOP;
    if (loop && st[S_BRKV]) {                        // u_hat was zero: v = 0 (vraw holds zeros), u stays
        for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j];
        return;
    }
    finalize(Pn, nbn, k + 2, h);
    const T sv = sqrt(h[k + 1]);
    T inv = T(1);
    if (mode != M_PLAIN) {
        if (!(sv > T(0))) {
            if (loop) {                              // deflation.hpp: sigma = 0 after the v-update -> break, v not normalised
                if (blockIdx.x == 0 && threadIdx.x == 0) st[S_BRKU] = 1;
                for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j];
                return;
            }
        } else {
            inv = T(1) / sv;
        }
        for (long j = (long)blockIdx.x * WG + threadIdx.x; j < n; j += (long)gridDim.x * WG) v[j] = vraw[j] * inv;
    }
    const T vsq = h[k + 1] * inv * inv * dc;
    const T sm = mu ? h[k] * inv : T(0);
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)m - r0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long i = r0 + r;
        T s = t[i] * inv - (mu ? mu[i] * sm : T(0));
        for (int q = 0; q < k; ++q) s -= U[(long)q * m + i] * (d[q] * (h[q] * inv));
        if (loop) s = regularize(s / vsq, l1, l2, nonneg, ub, vsq);
        xs[r] = s;
        uraw[i] = s;
    }
    __syncthreads();
    Cols<T> C;
    C.e[0] = uraw; C.e[1] = ucur; C.ne = 2;
    block_partials(xs, uraw, r0, cnt, C, Pu);
}

// End of one deflation iteration (m): sigma_u = |u_raw|; u = u_raw / sigma_u; convergence 1 - |u . u_old| < tol_k freezes the
// factor (st[S_STOP] = it + 1); iterations done -> st[S_ITERS] (the CPU's count: +1 on convergence, +0 on a break).
// Also prepares the next iteration: u_hat = u + beta (u - u_old) with the Nesterov beta of iteration it + 1 and its m-side
// partials [U_k' u_hat, mu . u_hat, |u_hat|^2] into Pm.
template <class T>
__global__ __launch_bounds__(WG) void defl_finish_kernel(const T* __restrict__ uraw, T* __restrict__ u, T* __restrict__ uhat, int m,
                                                         const T* __restrict__ Pu, int nbm, const T* __restrict__ U, int k,
                                                         const T* __restrict__ mu, T* __restrict__ Pm, T tol_k, int* st, int it) {
    if (idle(st, it)) return;
    __shared__ T h[2];
    __shared__ T xs[CH];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (st[S_BRKV] || st[S_BRKU]) {
        if (first) { st[S_ITERS] = it; st[S_STOP] = it + 1; }
        return;
    }
    finalize(Pu, nbm, 2, h);
    const T su = sqrt(h[0]);
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)m - r0);
    if (!(su > T(0))) {                              // u = 0 after the u-update: break with u unnormalised
        for (int r = threadIdx.x; r < cnt; r += WG) u[r0 + r] = uraw[r0 + r];
        if (first) { st[S_ITERS] = it; st[S_STOP] = it + 1; }
        return;
    }
    const T inv = T(1) / su;
    const bool conv = T(1) - fabs(h[1] * inv) < tol_k;
    const int nx = it + 1;
    const T beta = nx > 1 ? T(nx - 1) / T(nx + 2) : T(0);
    for (int r = threadIdx.x; r < cnt; r += WG) {
        const long i = r0 + r;
        const T un = uraw[i] * inv, uo = u[i];
        const T uh = un + beta * (un - uo);
        u[i] = un;
        uhat[i] = uh;
        xs[r] = uh;
    }
    if (first) { st[S_ITERS] = it + 1; if (conv) st[S_STOP] = it + 1; }
    if (conv) return;
    __syncthreads();
    Cols<T> C;
    C.X = U; C.ld = m; C.nx = k; C.e[0] = mu; C.e[1] = uhat; C.ne = 2;
    block_partials(xs, uhat, r0, cnt, C, Pm);
}

// One workgroup: Gram-Schmidt of x (len) against the first c columns of X, then |x| -> *norm_out and x /= |x| when |x| > thr.
// mgs = 1: sequential (modified) projections, one column at a time (deflation.hpp warm start);
// mgs = 0: two passes of classical GS, all c dots from the same x (deflation.hpp post-factor reorthogonalisation).
template <class T> __device__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    const int w = threadIdx.x / WAVE;
    __syncthreads();
    if (threadIdx.x % WAVE == 0) red[w] = v;
    __syncthreads();
    T s = 0;
    for (int q = 0; q < NW; ++q) s += red[q];
    return s;
}
template <class T>
__global__ __launch_bounds__(WG) void gs_kernel(T* __restrict__ x, long len, const T* __restrict__ X, int c, int mgs, T thr,
                                                T* __restrict__ norm_out) {
    __shared__ T red[NW];
    __shared__ T h[NPMAX];
    if (mgs) {
        for (int q = 0; q < c; ++q) {
            const T* col = X + (long)q * len;
            T a = 0;
            for (long i = threadIdx.x; i < len; i += WG) a += x[i] * col[i];
            const T dq = block_sum(a, red);
            for (long i = threadIdx.x; i < len; i += WG) x[i] -= dq * col[i];
            __syncthreads();
        }
    } else {
        for (int pass = 0; pass < 2 && c > 0; ++pass) {
            for (int q = 0; q < c; ++q) {
                const T* col = X + (long)q * len;
                T a = 0;
                for (long i = threadIdx.x; i < len; i += WG) a += col[i] * x[i];
                const T dq = block_sum(a, red);
                if (threadIdx.x == 0) h[q] = dq;
            }
            __syncthreads();
            for (long i = threadIdx.x; i < len; i += WG) {
                T s = 0;
                for (int q = 0; q < c; ++q) s += X[(long)q * len + i] * h[q];
                x[i] -= s;
            }
            __syncthreads();
        }
    }
    T a = 0;
    for (long i = threadIdx.x; i < len; i += WG) a += x[i] * x[i];
    const T nrm = sqrt(block_sum(a, red));
    if (nrm > thr) {
        const T inv = T(1) / nrm;
        for (long i = threadIdx.x; i < len; i += WG) x[i] *= inv;
    }
    if (norm_out && threadIdx.x == 0) *norm_out = nrm;
}

// ------------------------------------------------------------------------------------------------------------ Lanczos
// r = t - center * mu * sum(p_j) - beta_j q_{j-1}; partials against Q_j (j > 0) or |r|^2 (j = 0).
// Psum: partials of sum(p_j) (one column), read only when mu != nullptr.
template <class T>
__global__ __launch_bounds__(WG) void lz_r_kernel(const T* __restrict__ t, int m, const T* __restrict__ mu, const T* __restrict__ Psum,
                                                  int nbn, const T* __restrict__ beta, const T* __restrict__ Q, int j, T* __restrict__ r,
                                                  T* __restrict__ P, const int* st) {
    if (idle(st, j)) return;
    __shared__ T h[1];
    __shared__ T xs[CH];
    if (mu) finalize(Psum, nbn, 1, h);
    const T sp = mu ? h[0] : T(0);
    const T b = j > 0 ? beta[j] : T(0);
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)m - r0);
    for (int q = threadIdx.x; q < cnt; q += WG) {
        const long i = r0 + q;
        T s = t[i];
        if (mu) s -= mu[i] * sp;
        if (j > 0) s -= b * Q[(long)(j - 1) * m + i];
        xs[q] = s;
        r[i] = s;
    }
    __syncthreads();
    Cols<T> C;
    if (j > 0) { C.X = Q; C.ld = m; C.nx = j; } else { C.e[0] = r; C.ne = 1; }
    block_partials(xs, r, r0, cnt, C, P);
}
// s = y - center * (mu . q_j) - alpha_j p_j; partials against P_{j+1}.  Pmq: partials of mu . q_j.
template <class T>
__global__ __launch_bounds__(WG) void lz_s_kernel(const T* __restrict__ y, int n, const T* __restrict__ Pmq, int nbm, int center,
                                                  const T* __restrict__ alpha, const T* __restrict__ Pb, int j, T* __restrict__ s,
                                                  T* __restrict__ P, const int* st) {
    if (idle(st, j) || st[S_BRKV]) return;
    __shared__ T h[1];
    __shared__ T xs[CH];
    if (center) finalize(Pmq, nbm, 1, h);
    const T c = center ? h[0] : T(0), a = alpha[j];
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, (long)n - r0);
    for (int q = threadIdx.x; q < cnt; q += WG) {
        const long i = r0 + q;
        const T v = y[i] - c - a * Pb[(long)j * n + i];
        xs[q] = v;
        s[i] = v;
    }
    __syncthreads();
    Cols<T> C;
    C.X = Pb; C.ld = n; C.nx = j + 1;
    block_partials(xs, s, r0, cnt, C, P);
}
// one classical Gram-Schmidt pass: h = finalised partials (nx columns of X); x -= X h; then partials against X again (last = 0)
// or |x|^2 (last = 1)
template <class T>
__global__ __launch_bounds__(WG) void cgs_kernel(T* __restrict__ x, long len, const T* __restrict__ X, int nx, const T* __restrict__ Pin,
                                                 int nb, int last, T* __restrict__ Pout, const int* st, int j, int chk_brk) {
    if (idle(st, j) || (chk_brk && st[S_BRKV])) return;
    __shared__ T h[NPMAX];
    __shared__ T xs[CH];
    finalize(Pin, nb, nx, h);
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int q = threadIdx.x; q < cnt; q += WG) {
        const long i = r0 + q;
        T s = 0;
        for (int c = 0; c < nx; ++c) s += X[(long)c * len + i] * h[c];
        const T v = x[i] - s;
        xs[q] = v;
        x[i] = v;
    }
    __syncthreads();
    Cols<T> C;
    if (last) { C.e[0] = x; C.ne = 1; } else { C.X = X; C.ld = len; C.nx = nx; }
    block_partials(xs, x, r0, cnt, C, Pout);
}
// norm of x from its partials; below eps: lucky breakdown (side 0: alpha, step ends with j_actual = j; side 1: beta, j_actual =
// j + 1), else out = x / |x| and scal[idx] = |x|, and partials of out against e (mu . q_j or sum p_{j+1}; e_on = 0: none).
// side 1 ends the step: it records j + 1 steps done.
template <class T>
__global__ __launch_bounds__(WG) void lz_norm_kernel(const T* __restrict__ x, long len, const T* __restrict__ Pin, int nb, T eps,
                                                     const T* __restrict__ alpha0,
                                                     T* __restrict__ out, T* __restrict__ scal, int idx, int side, int e_on,
                                                     const T* __restrict__ e, T* __restrict__ Pout, int* st, int j) {
    if (idle(st, j) || (side == 1 && st[S_BRKV])) return;
    __shared__ T h[1];
    __shared__ T xs[CH];
    finalize(Pin, nb, 1, h);
    const T nrm = sqrt(h[0]);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    // breakdown threshold: 100 eps, scaled by alpha_0 (~ |A|) once it exists -- an absolute 100 eps misses the exhausted Krylov
    // space of a low-rank matrix in fp32, where the rounding noise of A p is ~ eps |A|
    const T thr = eps * ((side == 1 || j > 0) && alpha0[0] > T(1) ? alpha0[0] : T(1));
    if (!(nrm >= thr)) {
        if (first) {
            if (side == 0) st[S_BRKV] = 1;
            st[S_ITERS] = side == 0 ? j : j + 1;
            st[S_STOP] = j + 1;
        }
        return;
    }
    if (first) {
        scal[idx] = nrm;
        if (side == 1) st[S_ITERS] = j + 1;
    }
    const long r0 = (long)blockIdx.x * CH;
    const int cnt = (int)min((long)CH, len - r0);
    for (int q = threadIdx.x; q < cnt; q += WG) {
        const long i = r0 + q;
        const T v = x[i] / nrm;
        xs[q] = v;
        out[i] = v;
    }
    if (!e_on) return;
    __syncthreads();
    Cols<T> C;
    C.e[0] = e; C.ne = 1;
    block_partials(xs, out, r0, cnt, C, Pout);
}

// one term of a Ritz product.  ritz_kernel and nmf_start_kernel both accumulate through this function, from s = 0 over l ascending,
// so the compiler contracts (or does not contract) the multiply-add of both the same way and their sums agree bit for bit
template <class T> __device__ inline T ritz_step(T s, T b, T w) { return s + b * w; }

// out (len x kc, column-major) = B (len x ja) W (ja x kc): the Ritz vectors
template <class T>
__global__ __launch_bounds__(WG) void ritz_kernel(const T* __restrict__ B, long len, int ja, const T* __restrict__ W, int kc,
                                                  T* __restrict__ out) {
    const long i = (long)blockIdx.x * WG + threadIdx.x;
    const int c = blockIdx.y;
    if (i >= len || c >= kc) return;
    T s = 0;
    for (int l = 0; l < ja; ++l) s = ritz_step(s, B[(long)l * len + i], W[(long)c * ja + l]);
    out[(long)c * len + i] = s;
}

// The Ritz product written as an NMF start (nmf/nmf_init.hpp:71-79): out[i * k + c] = |sum_l B[l len + i] W[c ja + l]| * sq[c] for
// c < kc, sq[c] = sqrt(sigma_c) in T; out is row-major len x k, the column-major k x len factor the fit entries take.  Columns
// c >= kc of a row are not touched.
//   A thread owns row i and one chunk of NS_CW = 32 columns (blockIdx.y), whose sums it keeps in registers while it walks l once:
//   the basis is read ceil(kc / 32) times, not kc times.  32 accumulators are 32 VGPRs in fp32 and 64 in fp64; with the step's
//   staged coefficients the kernel takes 62 VGPRs in fp32 (8 waves a SIMD) and 127 in fp64 (4 waves), and nothing spills.  A chunk
//   of 64 would halve the basis reads again only from k = 65 on and leave fp64 two waves a SIMD.
//   The coefficients of the chunk sit in LDS, NS_LT = 64 steps of l at a time (W[l][c], every lane reads the same address: a
//   broadcast); tiles follow each other in l order, so the sum of (i, c) runs over l ascending exactly as ritz_kernel's.
//   The rows leave through LDS, NS_SC = 16 columns at a time (the tile reuses the coefficient storage): sixteen consecutive lanes
//   store sixteen consecutive values of one row, where a lane-per-row store would stride by k.
// No atomics and no dependence on the grid: two runs are bitwise equal.
constexpr int NS_CW = 32, NS_LT = 64, NS_SC = 16;
__device__ inline float ns_abs(float x) { return __builtin_fabsf(x); }
__device__ inline double ns_abs(double x) { return __builtin_fabs(x); }
template <class T>
__global__ __launch_bounds__(WG) void nmf_start_kernel(const T* __restrict__ B, long len, int ja, const T* __restrict__ W, int kc,
                                                       const T* __restrict__ sq, int k, T* __restrict__ out) {
    constexpr int LDS_W = NS_LT * NS_CW, LDS_T = WG * (NS_SC + 1);
    __shared__ T sh[LDS_W > LDS_T ? LDS_W : LDS_T];
    const long r0 = (long)blockIdx.x * WG;
    const long i = r0 + threadIdx.x;
    const long ic = i < len ? i : len - 1;             // a lane past the end reads the last row and stores nothing
    const int c0 = blockIdx.y * NS_CW;
    T acc[NS_CW];
#pragma unroll
    for (int c = 0; c < NS_CW; ++c) acc[c] = T(0);
    for (int l0 = 0; l0 < ja; l0 += NS_LT) {
        const int nl = min(NS_LT, ja - l0);
        __syncthreads();
        for (int q = threadIdx.x; q < nl * NS_CW; q += WG) {
            const int lt = q % nl, c = q / nl;          // consecutive threads read consecutive l of one column of W
            sh[lt * NS_CW + c] = c0 + c < kc ? W[(long)(c0 + c) * ja + l0 + lt] : T(0);
        }
        __syncthreads();
        for (int lt = 0; lt < nl; ++lt) {
            const T b = B[(long)(l0 + lt) * len + ic];
#pragma unroll
            for (int c = 0; c < NS_CW; ++c) acc[c] = ritz_step(acc[c], b, sh[lt * NS_CW + c]);
        }
    }
#pragma unroll
    for (int h = 0; h < NS_CW / NS_SC; ++h) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NS_SC; ++c) sh[threadIdx.x * (NS_SC + 1) + c] = acc[h * NS_SC + c];
        __syncthreads();
        for (int q = threadIdx.x; q < WG * NS_SC; q += WG) {
            const int r = q / NS_SC, c = q % NS_SC, cg = c0 + h * NS_SC + c;
            if (r0 + r < len && cg < kc) out[(r0 + r) * k + cg] = ns_abs(sh[r * (NS_SC + 1) + c]) * sq[cg];
        }
    }
}

}  // namespace rsv
