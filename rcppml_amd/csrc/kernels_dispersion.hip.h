// ============================================================================
// kernels_dispersion.hip.h -- dispersion estimators and per-element likelihoods of the IRLS losses for gfx950, and the pieces
// they share with their cross-validation counterparts (kernels_cv_irls.hip.h).
//
//   nb_size_rows_kernel     nmf/fit_cpu.hpp:1094-1265 (NB size, PER_ROW, sparse branch); <T, true> also returns the NB likelihood
//                           with the updated sizes (nmf/explicit_loss.hpp:53-77 + math/loss.hpp:415-426)
//   dispersion_rows_kernel  nmf/fit_cpu.hpp:914-1001 (GP theta, MM update), :1561-1661 (Gamma / inverse Gaussian / Tweedie phi)
//   vec_global_fill_kernel  GLOBAL dispersion: mean or the element nth_element puts at m / 2
//   nb_loss_lane_kernel     nmf/explicit_loss.hpp:53-77: per-element likelihoods over the nonzeros
//
// Row kernels: one wavefront per row i of A (= column i of A^T), one lane per nonzero; the row of W_T scaled by d sits in the
// wave's LDS slab (ScaledRow) and each lane dots it against its gathered row of H.  Column kernels: one wavefront per column j,
// one lane per entry; d and the column of H sit in LDS (stage_column) and each lane gathers its row of W_T (column_pred).
// The per-element terms themselves are dist_loss_term (kernels.hip.h).
// ============================================================================
#pragma once
#include "kernels_irls.hip.h"

namespace rk {

// acc <- step(acc, c, g[c]) for c = 0 .. k-1 in order, on ONE accumulator: g is read with 16-byte loads when vec_ok (k a multiple
// of the vector width, g 16-byte aligned) and element by element otherwise -- the same operations in the same order either way.
template <class T, class Step> __device__ __forceinline__ T gather_fold(const T* __restrict__ g, int k, bool vec_ok, Step step) {
    constexpr int VEC = 16 / sizeof(T);
    typedef typename VecT<T, VEC>::type V;
    T acc = T(0);
    if (vec_ok) {
        for (int c = 0; c < k; c += VEC) {
            const V v = *reinterpret_cast<const V*>(g + c);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc = step(acc, c + e, v[e]);
        }
    } else {
        for (int c = 0; c < k; ++c) acc = step(acc, c, g[c]);
    }
    return acc;
}
template <class T> __device__ __forceinline__ bool gather_vec_ok(const T* base, int k) {
    return (k % (16 / (int)sizeof(T)) == 0) && (reinterpret_cast<uintptr_t>(base) % 16 == 0);
}

// Row i of W_T scaled by d (apply_scaling(W_Td, d)): the lane keeps features lane and lane + 64 (k <= 128) and the whole row is
// parked in the wave's 128-element LDS slab, from where every lane reads it as a broadcast.
template <class T> struct ScaledRow {
    const T* slab;
    bool fok, fok2;
    int lane;
    T wd, wd2;
    __device__ __forceinline__ ScaledRow(T* slab_, const T* __restrict__ W_T, const T* __restrict__ d, int64_t i, int k, int lane_)
        : slab(slab_), fok(lane_ < k), fok2(lane_ + 64 < k), lane(lane_) {
        wd = fok ? W_T[i * (int64_t)k + lane] * d[lane] : T(0);
        wd2 = fok2 ? W_T[i * (int64_t)k + lane + 64] * d[lane + 64] : T(0);
        slab_[lane] = wd;
        slab_[lane + 64] = wd2;
        __builtin_amdgcn_wave_barrier();
    }
    // Wd_i . hr in feature order, in-lane (hr = this lane's gathered row of H)
    __device__ __forceinline__ T dot(const T* __restrict__ hr, int k, bool vec_ok) const {
        return gather_fold<T>(hr, k, vec_ok, [&](T acc, int c, T h) { return tfma(slab[c], h, acc); });
    }
    // Wd_i . v for a k-vector v (the Gram trick's row sums h_rs), by the whole wave
    __device__ __forceinline__ T dot_k(const T* __restrict__ v) const {
        return wave_sum((fok ? wd * v[lane] : T(0)) + (fok2 ? wd2 * v[lane + 64] : T(0)));
    }
    // Wd_i^T G Wd_i, fp64 accumulation as the reference, by the whole wave
    __device__ __forceinline__ double quad(const T* __restrict__ G, int k) const {
        double acc = 0.0;
        for (int b2 = 0; b2 < k; ++b2) {
            const double wb = static_cast<double>(slab[b2]);
            if (fok) acc += static_cast<double>(wd) * static_cast<double>(G[(int64_t)b2 * k + lane]) * wb;
            if (fok2) acc += static_cast<double>(wd2) * static_cast<double>(G[(int64_t)b2 * k + lane + 64]) * wb;
        }
        return wave_sum(acc);
    }
};

// nmf/fit_cpu.hpp:1230-1252  the method-of-moments NB size of one row from its fp64 sums; `size` keeps its value when the
// quotient is not finite
template <class T> __device__ __forceinline__ void nb_moment_size(double s_mu2, double s_res2, double total_mu, double total_mu_sq,
                                                                  double r_min, double r_max, T& size) {
    const double total_resid_sq = s_res2 + (total_mu_sq - s_mu2);
    const double excess = total_resid_sq - total_mu;
    if (excess > 1e-10 && total_mu_sq > 1e-10) {
        double r_new = total_mu_sq / excess;
        r_new = r_new < r_max ? r_new : r_max;
        r_new = r_new > r_min ? r_new : r_min;
        if (isfinite(r_new)) size = static_cast<T>(r_new);
    } else {
        size = static_cast<T>(r_max);
    }
}

// NB size (r) method-of-moments update, one wavefront per ROW i of A: nonzero sums of mu^2 and (y-mu)^2 in fp64, totals via
// Wd_i . h_rs  and  Wd_i^T G_H Wd_i.
// WITH_LOSS (PER_ROW dispersion, no robust modifier; what the fit loop runs): also the NB negative log-likelihood with the UPDATED
// sizes, as the fit loop orders them.  The first pass parks every prediction in mu_cache (each lane re-reads only what it wrote);
// the row's new size is known to the whole wave (wave_sum leaves the same sums in all lanes), and a second pass evaluates the
// likelihood terms from the parked predictions -- no second gather of factor rows, and lgamma(r_i) once per row instead of once per
// nonzero.  The terms are those of nb_loss_lane_kernel (same prediction arithmetic: (W d) . H in feature order, same fp64
// formula, each term cast to Scalar); only the order of the fp64 sum differs (by row instead of by column).
template <class T, bool WITH_LOSS>
__global__ __launch_bounds__(256) void nb_size_rows_kernel(
    const int* __restrict__ tp, const int* __restrict__ ti, const T* __restrict__ tx, int64_t m,
    const T* __restrict__ W_T, const T* __restrict__ d, const T* __restrict__ H, const T* __restrict__ h_rs,
    const T* __restrict__ G_H, int k, double r_min, double r_max, T* __restrict__ nb_size, T* __restrict__ mu_cache,
    double* __restrict__ partial) {
    __shared__ T wds[4][128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    double nll_sum = 0.0;
    if (i < m) {
        const ScaledRow<T> row(wds[wave], W_T, d, i, k, lane);
        const bool vec_ok = gather_vec_ok(H, k);
        const int ts = tp[i], te = tp[i + 1];
        double s_mu2 = 0.0, s_res2 = 0.0;
        for (int t = ts + lane; t < te; t += 64) {
            const T dot = row.dot(H + (int64_t)ti[t] * k, k, vec_ok);
            if constexpr (WITH_LOSS) mu_cache[t] = dot;
            const double y = static_cast<double>(tx[t]);
            double mu = static_cast<double>(dot);
            mu = mu > 1e-10 ? mu : 1e-10;
            const double resid = y - mu;
            s_mu2 += mu * mu;
            s_res2 += resid * resid;
        }
        s_mu2 = wave_sum(s_mu2);
        s_res2 = wave_sum(s_res2);
        const double total_mu = static_cast<double>(row.dot_k(h_rs));
        const double total_mu_sq = row.quad(G_H, k);
        T size_new = nb_size[i];
        nb_moment_size(s_mu2, s_res2, total_mu, total_mu_sq, r_min, r_max, size_new);
        if (lane == 0) nb_size[i] = size_new;
        if constexpr (WITH_LOSS) {               // likelihood terms of the row with the updated size (math/loss.hpp:415-426)
            const double th = static_cast<double>(size_new);
            const double r = th > 1e-10 ? th : 1e-10;
            const double lg_r = lgamma(r);
            for (int t = ts + lane; t < te; t += 64) {
                const double y = static_cast<double>(tx[t]);
                double mu = static_cast<double>(mu_cache[t]);
                mu = mu > 1e-10 ? mu : 1e-10;
                nll_sum += static_cast<double>(static_cast<T>(nb_loss_term(y, mu, r, lg_r)));    // the reference casts each term to Scalar
            }
        }
    }
    if constexpr (WITH_LOSS) {
        __shared__ double sh[4];
        nll_sum = wave_sum(nll_sum);
        if (lane == 0) sh[wave] = nll_sum;
        __syncthreads();
        if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
    }
}

// GP theta, auxiliary-function (MM) update of one row (nmf/fit_cpu.hpp:940-1001; fit_cv.hpp:905-961): five inner passes over the
// row's parked predictions accumulate alpha / gamma in fp64, theta rounded through Scalar between passes, as the reference.
// SKIP_HELD (cross-validation only): an entry parked as a negative number is held out and takes no part.  The plain update
// parks raw predictions, which may be negative when nonneg is off, and must not skip them.
template <class T, bool SKIP_HELD>
__device__ __forceinline__ T gp_theta_mm(const T* __restrict__ tx, const T* __restrict__ s_cache, int ts, int te, int lane,
                                         double sum_y, double n_nz, double sum_s, double hi, T th_s) {
    for (int mm = 0; mm < 5; ++mm) {                                                          // THETA_INNER_ITERS
        const double th = static_cast<double>(th_s);
        double alpha = 0.0, gamma = 0.0;
        for (int t = ts + lane; t < te; t += 64) {
            const double y = static_cast<double>(tx[t]);
            if (y >= 1.0) {
                const T sc = s_cache[t];
                if (SKIP_HELD && sc < T(0)) continue;
                double sv = static_cast<double>(sc);
                sv = sv > 1e-10 ? sv : 1e-10;
                double denom = sv + th * y;
                denom = denom > 1e-10 ? denom : 1e-10;
                const double eta1 = sv / denom;
                alpha += (y - 1.0) * eta1;
                gamma += (y - 1.0) * (1.0 - eta1);
            }
        }
        alpha = wave_sum(alpha);
        gamma = wave_sum(gamma);
        const double a = alpha + n_nz;
        const double b = (sum_y - sum_s) - gamma + a;
        if (a > 1e-15) {
            const double disc = b * b + 4.0 * a * gamma;
            if (disc > 0.0 && isfinite(disc)) {
                const double nt = (-b + sqrt(disc)) / (2.0 * a);
                if (isfinite(nt) && nt >= 0.0) th_s = static_cast<T>(nt < hi ? nt : hi);
            }
        }
    }
    return th_s;
}

// Dispersion estimators of the other IRLS losses, one wavefront per ROW i of A, one lane per nonzero:
//   loss_type 4      GP theta: the Scalar predictions s of the row's nonzeros are parked in s_cache (each lane re-reads what it
//                    wrote), then gp_theta_mm;
//   loss_type 6/7/8  Pearson phi over the positive nonzeros, nmf/fit_cpu.hpp:1561-1661, clamped to [lo, hi].
template <class T>
__global__ __launch_bounds__(256) void dispersion_rows_kernel(
    const int* __restrict__ tp, const int* __restrict__ ti, const T* __restrict__ tx, int64_t m,
    const T* __restrict__ W_T, const T* __restrict__ d, const T* __restrict__ H, const T* __restrict__ h_rs, int k,
    int loss_type, double power, double lo, double hi, T* __restrict__ s_cache, T* __restrict__ theta) {
    __shared__ T wds[4][128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= m) return;
    const ScaledRow<T> row(wds[wave], W_T, d, i, k, lane);
    const bool vec_ok = gather_vec_ok(H, k);
    const int ts = tp[i], te = tp[i + 1];
    const bool is_gp = loss_type == 4;
    const double var_power = loss_type == 8 ? power : (loss_type == 6 ? 2.0 : 3.0);
    double acc0 = 0.0, acc1 = 0.0;      // GP: sum_y, n_nz      phi: sum of Pearson terms, count
    for (int t = ts + lane; t < te; t += 64) {
        const T dot = row.dot(H + (int64_t)ti[t] * k, k, vec_ok);
        const double y = static_cast<double>(tx[t]);
        if (is_gp) {
            s_cache[t] = dot;
            acc0 += y;
            if (y >= 1.0) acc1 += 1.0;
        } else if (y > 0.0) {
            double mu = static_cast<double>(dot);
            mu = mu > 1e-10 ? mu : 1e-10;
            const double resid = y - mu;
            double v_mu = pow(mu, var_power);
            v_mu = v_mu > 1e-20 ? v_mu : 1e-20;
            acc0 += (resid * resid) / v_mu;
            acc1 += 1.0;
        }
    }
    acc0 = wave_sum(acc0);
    acc1 = wave_sum(acc1);
    if (!is_gp) {
        if (lane == 0 && acc1 > 0.0) {
            double pn = acc0 / acc1;
            pn = pn < hi ? pn : hi;
            pn = pn > lo ? pn : lo;
            if (isfinite(pn)) theta[i] = static_cast<T>(pn);
        }
        return;
    }
    const double sum_s = static_cast<double>(row.dot_k(h_rs));                                // Gram trick, :935-938
    const T th_s = gp_theta_mm<T, false>(tx, s_cache, ts, te, lane, acc0, acc1, sum_s, hi, theta[i]);
    if (lane == 0) theta[i] = th_s;
}

// GLOBAL dispersion: every entry <- the mean (stat 0; GP, fit_cpu.hpp:1005-1008) or <- src[m/2] of the SORTED copy
// (stat 1: nth_element at m/2; NB :1257-1262, phi :1664-1669).  Single block.
// The median is found by an 8-bit radix SELECT on order-preserving integer keys (no sort: the reference only needs the element
// nth_element would put at m / 2): per digit, a 256-bin histogram of the candidates that share the prefix found so far.
template <class T> struct OrdKey;
template <> struct OrdKey<float> {
    typedef unsigned int U;
    static __device__ __forceinline__ U enc(float v) { const U b = __float_as_uint(v); return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
    static __device__ __forceinline__ float dec(U k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
};
template <> struct OrdKey<double> {
    typedef unsigned long long U;
    static __device__ __forceinline__ U enc(double v) { const U b = (U)__double_as_longlong(v); return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull); }
    static __device__ __forceinline__ double dec(U k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull))); }
};
template <class T>
__global__ __launch_bounds__(256) void vec_global_fill_kernel(T* __restrict__ x, int64_t m, int stat) {
    __shared__ double red[256];
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long sel[2];              // [0] = digit chosen, [1] = rank left inside it
    T val;
    if (stat == 1) {
        typedef typename OrdKey<T>::U U;
        U prefix = 0, mask = 0;
        unsigned long long kth = (unsigned long long)(m / 2);      // 0-based rank of the wanted element
        for (int shift = (int)sizeof(U) * 8 - 8; shift >= 0; shift -= 8) {
            hist[threadIdx.x] = 0;
            __syncthreads();
            for (int64_t i = threadIdx.x; i < m; i += 256) {
                const U key = OrdKey<T>::enc(x[i]);
                if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)((key >> shift) & 0xff)], 1u);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long run = 0;
                int dgt = 0;
                for (; dgt < 255; ++dgt) {
                    if (run + hist[dgt] > kth) break;
                    run += hist[dgt];
                }
                sel[0] = (unsigned long long)dgt;
                sel[1] = kth - run;
            }
            __syncthreads();
            prefix |= (U)sel[0] << shift;
            mask |= (U)0xff << shift;
            kth = sel[1];
            __syncthreads();
        }
        val = OrdKey<T>::dec(prefix);
    } else {
        double acc = 0.0;
        for (int64_t i = threadIdx.x; i < m; i += 256) acc += static_cast<double>(x[i]);
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        val = static_cast<T>(red[0] / static_cast<double>(m));
    }
    __syncthreads();
    for (int64_t i = threadIdx.x; i < m; i += 256) x[i] = val;
}

// Column side: d (block-wide) and column j of H (one slab per wave) into LDS, zero-padded to 128 features; ends in a block barrier.
template <class T>
__device__ __forceinline__ void stage_column(T (&dsh)[128], T (&hs)[4][128], const T* __restrict__ d, const T* __restrict__ H,
                                             int64_t j, int64_t ncols, int k) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < 128) dsh[threadIdx.x] = (int)threadIdx.x < k ? d[threadIdx.x] : T(0);
    hs[wave][lane] = (j < ncols && lane < k) ? H[j * (int64_t)k + lane] : T(0);
    hs[wave][lane + 64] = (j < ncols && lane + 64 < k) ? H[j * (int64_t)k + lane + 64] : T(0);
    __syncthreads();
}
// pred = sum_c (W_T(row, c) d_c) H_c in feature order, in-lane (wr = this lane's gathered row of W_T)
template <class T>
__device__ __forceinline__ T column_pred(const T* __restrict__ wr, const T* dsh, const T* hs, int k, bool vec_ok) {
    return gather_fold<T>(wr, k, vec_ok, [&](T acc, int c, T w) { return tfma(w * dsh[c], hs[c], acc); });
}

// math/loss.hpp:549-607  compute_robust_loss: Huber rho of the Pearson residual, in Scalar arithmetic
template <class T> __device__ __forceinline__ T robust_loss_term(int loss_type, T observed, T predicted, T theta, double power, double robust) {
    const T muS = predicted > T(1e-10) ? predicted : T(1e-10);
    const T resid = observed - muS;
    T var_mu;
    if (loss_type == 4 || loss_type == 3) var_mu = muS;
    else if (loss_type == 5) { const T r = theta > T(1e-10) ? theta : T(1e-10); var_mu = muS + muS * muS / r; }
    else if (loss_type == 6) var_mu = muS * muS;
    else if (loss_type == 7) var_mu = muS * muS * muS;
    else if (loss_type == 8) var_mu = static_cast<T>(pow(static_cast<double>(muS), power));
    else var_mu = T(1);
    const T sd = sqrt(var_mu > T(1e-20) ? var_mu : T(1e-20));
    const T pr = resid / sd;
    const T apr = tabs(pr);
    const T dl = static_cast<T>(robust);
    return apr <= dl ? T(0.5) * pr * pr : dl * apr - T(0.5) * dl * dl;
}

// Negative log-likelihood / deviance over the NONZEROS of A (explicit_loss.hpp:53-77), per-row theta, fp64 partials.
// One wavefront per column, ONE LANE PER NONZERO: each lane gathers its row of W_T, forms the prediction as k in-lane fmas
// against the column of H (broadcast from LDS) and evaluates the lgamma / log terms of its own nonzero -- 64 likelihood terms
// per wave instruction stream instead of one.
template <class T>
__global__ __launch_bounds__(256) void nb_loss_lane_kernel(
    const int* __restrict__ colptr, const int* __restrict__ rowidx, const T* __restrict__ vals, int64_t ncols,
    const T* __restrict__ W_T, const T* __restrict__ d, const T* __restrict__ H, const T* __restrict__ theta_row, int k,
    int loss_type, double power, double robust, double* __restrict__ partial) {
    __shared__ double sh[4];
    __shared__ T hs[4][128];
    __shared__ T dsh[128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    stage_column(dsh, hs, d, H, j, ncols, k);
    double acc = 0.0;
    if (j < ncols) {
        const bool vec_ok = gather_vec_ok(W_T, k);
        const int as = colptr[j], ae = colptr[j + 1];
        for (int t = as + lane; t < ae; t += 64) {
            const int row = rowidx[t];
            const T pred = column_pred(W_T + (int64_t)row * k, dsh, hs[wave], k, vec_ok);
            const T th = theta_row ? theta_row[row] : T(0);
            double nll;
            if (robust > 0.0) {
                nll = static_cast<double>(robust_loss_term<T>(loss_type, vals[t], pred, th, power, robust));
            } else {
                double mu = static_cast<double>(pred);
                mu = mu > 1e-10 ? mu : 1e-10;
                nll = dist_loss_term(loss_type, static_cast<double>(vals[t]), mu, static_cast<double>(th), power);
            }
            acc += static_cast<double>(static_cast<T>(nll));      // the reference casts each term to Scalar
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

}  // namespace rk
