// ops_distribution.hip -- the distribution diagnostics of the reference's R/auto_distribution.R on the device (kernels:
// kernels_distribution.hip.h): rcppml_gpu_score_test_double, rcppml_gpu_zero_inflation_double and rcppml_gpu_dispersion_double.
// R forms (W %*% diag(d)) %*% H as a dense m x n matrix on the host; here mu is formed a tile at a time and reduced in the same
// kernel.  The one m x n array is phi of the dispersion entry (its trimmed means need every value).  The decisions R takes on the
// host (labels, which.min, the modes, the cvs) stay with the caller (rcppml_amd/distribution.py).
//
// The matrix is a CSC (col_ptr, row_idx, values, nnz) or a column-major dense array: exactly one of the two.  The model is W_T
// (k x m), d (k) and H (k x n).  Every entry refuses a call (*out_status = -1, reason in rcppml_gpu_last_error, no output written)
// on m, n or k below 1, both or neither matrix forms, a malformed CSC (rows strictly increasing within a column: the dgCMatrix
// invariant, and what keeps the per-nonzero overwrite of phi race-free), non-finite values in the matrix or the model, arguments
// outside their range, a call that does not fit in free device memory (the message gives the byte count), or no device.
#include "entry_common.hip.h"
#include "kernels_distribution.hip.h"

#include <cmath>
#include <string>
#include <vector>

namespace {
using namespace rcppml_plugin;
using namespace rdist;

struct In {
    const int* p = nullptr;
    const int* i = nullptr;
    const double* x = nullptr;
    int64_t nnz = 0;
    const double* dense = nullptr;
    int64_t m = 0, n = 0;
    int k = 0;
    const double *W_T = nullptr, *d = nullptr, *H = nullptr;
};

In read_in(const int* col_ptr, const int* row_idx, const double* values, const int* nnz, const double* dense, const int* m,
           const int* n, const int* k, const double* W_T, const double* d, const double* H) {
    if (!m || !n || !k) throw std::invalid_argument("null scalar argument");
    if (*m < 1 || *n < 1 || *k < 1) throw std::invalid_argument("m, n and k must be >= 1");
    if (col_ptr && dense) throw std::invalid_argument("give the matrix either as a CSC or as a dense array, not both");
    if (!col_ptr && !dense) throw std::invalid_argument("give the matrix as a CSC or as a dense array");
    if (!W_T || !d || !H) throw std::invalid_argument("null model array");
    In in;
    in.m = *m; in.n = *n; in.k = *k; in.W_T = W_T; in.d = d; in.H = H;
    if (col_ptr) {
        if (!nnz || *nnz < 0) throw std::invalid_argument("nnz must be >= 0");
        if (*nnz > 0 && (!row_idx || !values)) throw std::invalid_argument("null CSC array");
        in.p = col_ptr; in.i = row_idx; in.x = values; in.nnz = *nnz;
        check_csc_strict(col_ptr, row_idx, in.m, in.n, in.nnz);
        all_finite(values, (size_t)in.nnz, "the matrix");
    } else {
        in.dense = dense;
        all_finite(dense, (size_t)(in.m * in.n), "the matrix");
    }
    all_finite(W_T, (size_t)in.k * in.m, "W");
    all_finite(d, (size_t)in.k, "d");
    all_finite(H, (size_t)in.k * in.n, "H");
    return in;
}

size_t model_bytes(const In& in) { return 8 * ((size_t)in.k * (size_t)(2 * in.m + in.n) + in.k); }
size_t matrix_bytes(const In& in) {
    return in.dense ? 8 * (size_t)(in.m * in.n) : (size_t)(in.n + 1) * 4 + (size_t)in.nnz * 12;
}

// The matrix and the model on the device; a = W_T * d formed on the host (R's W %*% diag(d), one rounding per element).
struct Dev {
    DevBuf p, i, x, X, A, W, d, H;
    MuArgs args{};
    int64_t ntr = 0, ntc = 0;
    Dev(const In& in, hipStream_t s) {
        std::vector<double> a((size_t)in.k * in.m);
        for (int64_t r = 0; r < in.m; ++r)
            for (int f = 0; f < in.k; ++f) a[(size_t)r * in.k + f] = in.W_T[(size_t)r * in.k + f] * in.d[f];
        args.A = upload(A, a.data(), a.size(), s);
        args.H = upload(H, in.H, (size_t)in.k * in.n, s);
        upload(W, in.W_T, (size_t)in.k * in.m, s);
        upload(d, in.d, (size_t)in.k, s);
        if (in.dense) {
            args.X = upload(X, in.dense, (size_t)(in.m * in.n), s);
        } else {
            upload(p, in.p, (size_t)in.n + 1, s);
            upload(i, in.i, (size_t)in.nnz, s);
            upload(x, in.x, (size_t)in.nnz, s);
        }
        args.m = in.m; args.n = in.n; args.k = in.k;
        ntr = (in.m + TM - 1) / TM;
        ntc = (in.n + TN - 1) / TN;
        if (ntr * ntc >= ((int64_t)1 << 31)) throw std::invalid_argument("m x n is too large for the tile grid");
        args.ntr = (int)ntr;
        // the host buffer `a` goes out of scope: finish its copy first
        HIPCHK(hipStreamSynchronize(s));
    }
    unsigned tiles() const { return (unsigned)(ntr * ntc); }
    unsigned col_wave_blocks() const { return (unsigned)((args.n + 3) / 4); }
};

// R's mean(x, trim): lo = floor(N * trim) + 1, hi = N + 1 - lo
void trim_bounds(int64_t N, double trim, long long& lo, long long& hi) {
    lo = (long long)std::floor((double)N * trim) + 1;
    hi = (long long)N + 1 - lo;
}

constexpr int kGlobBlocks = 2048;

}  // namespace

extern "C" void rcppml_gpu_score_test_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
                                             const double* dense, int* m, int* n, int* k, const double* W_T, const double* d,
                                             const double* H, const double* powers, int* n_powers, double* min_mu,
                                             double* out_T, double* out_T_nb, int* out_all_integer, int64_t* out_count,
                                             int* out_status) {
    entry_guard(out_status, [&] {
        const In in = read_in(col_ptr, row_idx, values, nnz, dense, m, n, k, W_T, d, H);
        if (!n_powers || *n_powers < 1 || *n_powers > MAXP)
            throw std::invalid_argument("n_powers must be in [1, " + std::to_string(MAXP) + "]");
        if (!powers || !min_mu) throw std::invalid_argument("null argument");
        all_finite(powers, (size_t)*n_powers, "powers");
        if (!std::isfinite(*min_mu)) throw std::invalid_argument("min_mu must be finite");
        if (!out_T || !out_T_nb || !out_all_integer || !out_count) throw std::invalid_argument("null output");
        const int np = *n_powers;
        const int64_t nblk = in.dense ? ((in.m + TM - 1) / TM) * ((in.n + TN - 1) / TN) : (in.n + 3) / 4;
        device_ready(model_bytes(in) + matrix_bytes(in) + (size_t)nblk * (np + 1) * 8 + 4096);
        Stream st;
        Dev D(in, st.s);
        DevBuf part, sums, cnt;
        D.args.npow = np;
        for (int q = 0; q < np; ++q) D.args.pw[q] = powers[q];
        D.args.min_mu = *min_mu;
        D.args.part = zeros<double>(part, (size_t)nblk * (np + 1), st.s);
        unsigned long long* dcnt = zeros<unsigned long long>(cnt, 2, st.s);
        D.args.nonint = dcnt + 1;
        if (in.dense) {
            hipLaunchKernelGGL(mu_tile_kernel<MODE_SCORE>, dim3(D.tiles()), dim3(NT), 0, st.s, D.args);
        } else {
            hipLaunchKernelGGL(nz_kernel<MODE_SCORE>, dim3(D.col_wave_blocks()), dim3(NT), 0, st.s, D.p.as<int>(), D.i.as<int>(),
                               D.x.as<double>(), D.W.as<double>(), D.d.as<double>(), D.H.as<double>(), D.args, dcnt);
        }
        HIPCHK(hipGetLastError());
        zeros<double>(sums, (size_t)np + 1, st.s);
        hipLaunchKernelGGL(sum_block_partials, dim3(1), dim3(NT), 0, st.s, D.args.part, nblk, np + 1, sums.as<double>());
        HIPCHK(hipGetLastError());
        std::vector<double> s((size_t)np + 1);
        unsigned long long c[2];
        download(s.data(), sums.as<double>(), s.size(), st.s);
        download(c, cnt.as<unsigned long long>(), 2, st.s);
        const double count = in.dense ? (double)in.m * (double)in.n : (double)c[0];
        for (int q = 0; q < np; ++q) out_T[q] = s[q] / count;
        *out_T_nb = s[np] / count;
        *out_all_integer = c[1] == 0 ? 1 : 0;
        *out_count = in.dense ? in.m * in.n : (int64_t)c[0];
    });
}

extern "C" void rcppml_gpu_zero_inflation_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
                                                 const double* dense, int* m, int* n, int* k, const double* W_T, const double* d,
                                                 const double* H, double* out_expected_row, double* out_expected_col,
                                                 double* out_observed_row, double* out_observed_col, int* out_status) {
    entry_guard(out_status, [&] {
        const In in = read_in(col_ptr, row_idx, values, nnz, dense, m, n, k, W_T, d, H);
        if (!out_expected_row || !out_expected_col || !out_observed_row || !out_observed_col)
            throw std::invalid_argument("null output");
        const int64_t ntr = (in.m + TM - 1) / TM, ntc = (in.n + TN - 1) / TN;
        device_ready(model_bytes(in) + matrix_bytes(in) + 8 * (size_t)(ntc * in.m + ntr * in.n) + 16 * (size_t)(in.m + in.n) + 4096);
        Stream st;
        Dev D(in, st.s);
        DevBuf prow, pcol, erow, ecol, zrow, zcol;
        D.args.prow = zeros<double>(prow, (size_t)(ntc * in.m), st.s);
        D.args.pcol = zeros<double>(pcol, (size_t)(ntr * in.n), st.s);
        if (in.dense) {
            D.args.zrow = zeros<unsigned long long>(zrow, (size_t)in.m, st.s);
            D.args.zcol = zeros<unsigned long long>(zcol, (size_t)in.n, st.s);
        }
        hipLaunchKernelGGL(mu_tile_kernel<MODE_ZI>, dim3(D.tiles()), dim3(NT), 0, st.s, D.args);
        HIPCHK(hipGetLastError());
        erow.alloc((size_t)in.m * 8);
        ecol.alloc((size_t)in.n * 8);
        hipLaunchKernelGGL(sum_strided_partials, dim3((unsigned)((in.m + NT - 1) / NT)), dim3(NT), 0, st.s, D.args.prow, ntc, in.m,
                           erow.as<double>());
        hipLaunchKernelGGL(sum_strided_partials, dim3((unsigned)((in.n + NT - 1) / NT)), dim3(NT), 0, st.s, D.args.pcol, ntr, in.n,
                           ecol.as<double>());
        HIPCHK(hipGetLastError());
        std::vector<double> er((size_t)in.m), ec((size_t)in.n), orow((size_t)in.m), ocol((size_t)in.n);
        download(er.data(), erow.as<double>(), er.size(), st.s);
        download(ec.data(), ecol.as<double>(), ec.size(), st.s);
        if (in.dense) {
            std::vector<unsigned long long> zr((size_t)in.m), zc((size_t)in.n);
            download(zr.data(), zrow.as<unsigned long long>(), zr.size(), st.s);
            download(zc.data(), zcol.as<unsigned long long>(), zc.size(), st.s);
            for (int64_t r = 0; r < in.m; ++r) orow[r] = (double)zr[r];
            for (int64_t j = 0; j < in.n; ++j) ocol[j] = (double)zc[j];
        } else {
            // m - diff(p) per column, n - tabulate(i) per row: every stored entry counts as a nonzero, explicit zeros included
            std::vector<int64_t> rnz((size_t)in.m, 0);
            for (int64_t e = 0; e < in.nnz; ++e) ++rnz[in.i[e]];
            for (int64_t r = 0; r < in.m; ++r) orow[r] = (double)(in.n - rnz[r]);
            for (int64_t j = 0; j < in.n; ++j) ocol[j] = (double)(in.m - (in.p[j + 1] - in.p[j]));
        }
        std::copy(er.begin(), er.end(), out_expected_row);
        std::copy(ec.begin(), ec.end(), out_expected_col);
        std::copy(orow.begin(), orow.end(), out_observed_row);
        std::copy(ocol.begin(), ocol.end(), out_observed_col);
    });
}

extern "C" void rcppml_gpu_dispersion_double(const int* col_ptr, const int* row_idx, const double* values, int* nnz,
                                             const double* dense, int* m, int* n, int* k, const double* W_T, const double* d,
                                             const double* H, double* power, double* min_mu, double* trim, double* out_row_phi,
                                             double* out_col_phi, double* out_global_phi, int* out_status) {
    entry_guard(out_status, [&] {
        const In in = read_in(col_ptr, row_idx, values, nnz, dense, m, n, k, W_T, d, H);
        if (!power || !min_mu || !trim) throw std::invalid_argument("null argument");
        if (!std::isfinite(*power)) throw std::invalid_argument("power must be finite");
        if (!std::isfinite(*min_mu)) throw std::invalid_argument("min_mu must be finite");
        if (!(*trim >= 0.0 && *trim < 0.5)) throw std::invalid_argument("trim must lie in [0, 0.5)");
        if (!out_row_phi || !out_col_phi || !out_global_phi) throw std::invalid_argument("null output");
        const int64_t mn = in.m * in.n;
        device_ready(model_bytes(in) + matrix_bytes(in) + 8 * (size_t)mn + 8 * (size_t)(in.m + in.n) +
                     (size_t)kGlobBlocks * 24 + 8192);
        Stream st;
        Dev D(in, st.s);
        DevBuf phi, rphi, cphi, gphi, state, hist, psum, pcnt;
        phi.alloc((size_t)mn * 8);
        D.args.phi = phi.as<double>();
        D.args.power = *power;
        D.args.min_mu = *min_mu;
        hipLaunchKernelGGL(mu_tile_kernel<MODE_DISP>, dim3(D.tiles()), dim3(NT), 0, st.s, D.args);
        HIPCHK(hipGetLastError());
        if (!in.dense && in.nnz > 0) {
            hipLaunchKernelGGL(nz_kernel<MODE_DISP>, dim3(D.col_wave_blocks()), dim3(NT), 0, st.s, D.p.as<int>(), D.i.as<int>(),
                               D.x.as<double>(), D.W.as<double>(), D.d.as<double>(), D.H.as<double>(), D.args, nullptr);
            HIPCHK(hipGetLastError());
        }
        long long lo, hi;
        // per column: m contiguous values
        trim_bounds(in.m, *trim, lo, hi);
        cphi.alloc((size_t)in.n * 8);
        hipLaunchKernelGGL(seg_trim_kernel<1>, dim3((unsigned)in.n), dim3(NT), 0, st.s, D.args.phi, in.n, in.m, (int64_t)1, in.m, lo,
                           hi, cphi.as<double>());
        HIPCHK(hipGetLastError());
        // per row: n values at stride m, 16 rows per workgroup
        trim_bounds(in.n, *trim, lo, hi);
        rphi.alloc((size_t)in.m * 8);
        hipLaunchKernelGGL(seg_trim_kernel<16>, dim3((unsigned)((in.m + 15) / 16)), dim3(NT), 0, st.s, D.args.phi, in.m, (int64_t)1,
                           in.m, in.n, lo, hi, rphi.as<double>());
        HIPCHK(hipGetLastError());
        // all m * n values
        trim_bounds(mn, *trim, lo, hi);
        const GSel g0{{0ull, 0ull}, {lo, hi}};
        upload(state, &g0, 1, st.s);
        unsigned long long* dh = zeros<unsigned long long>(hist, 512, st.s);
        const int gb = (int)std::min<int64_t>(kGlobBlocks, (mn + NT - 1) / NT);
        for (int shift = 56; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(glob_hist_kernel, dim3((unsigned)gb), dim3(NT), 0, st.s, D.args.phi, mn, shift, state.as<GSel>(), dh);
            hipLaunchKernelGGL(glob_choose_kernel, dim3(1), dim3(64), 0, st.s, state.as<GSel>(), dh, shift);
        }
        psum.alloc((size_t)gb * 8);
        pcnt.alloc((size_t)gb * 16);
        gphi.alloc(8);
        hipLaunchKernelGGL(glob_sum_kernel, dim3((unsigned)gb), dim3(NT), 0, st.s, D.args.phi, mn, state.as<GSel>(), psum.as<double>(),
                           pcnt.as<long long>());
        hipLaunchKernelGGL(glob_final_kernel, dim3(1), dim3(NT), 0, st.s, psum.as<double>(), pcnt.as<long long>(), gb,
                           state.as<GSel>(), lo, hi, gphi.as<double>());
        HIPCHK(hipGetLastError());
        std::vector<double> rp((size_t)in.m), cp((size_t)in.n);
        double gv = 0;
        download(rp.data(), rphi.as<double>(), rp.size(), st.s);
        download(cp.data(), cphi.as<double>(), cp.size(), st.s);
        download(&gv, gphi.as<double>(), 1, st.s);
        std::copy(rp.begin(), rp.end(), out_row_phi);
        std::copy(cp.begin(), cp.end(), out_col_phi);
        *out_global_phi = gv;
    });
}
