// ops_similarity.hip -- column similarities and factor matching (kernels: kernels_similarity.hip.h) and their build-defined entries:
// rcppml_gpu_cosine_sparse_ex (every column of a CSC matrix against every column of another, dense result),
// rcppml_gpu_cosine_dense_ex (a stack of factor matrices against one reference, cosine or Pearson correlation),
// rcppml_gpu_bipartite_match_ex (minimum-cost assignment on the host, no device) and rcppml_gpu_cosine_geometry.  They are the
// compute side of the reference's cosine(), bipartiteMatch() and align() (R/cosine.R, R/bipartiteMatch.R, R/nmf_methods.R:261-271).
//
// Every argument is checked before the device is touched, and outputs are written only after the device work has succeeded, so a
// refused call leaves every output buffer as it was.
#include "entry_common.hip.h"
#include "kernels_similarity.hip.h"

#include <chrono>
#include <climits>
#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace {
using namespace rcppml_plugin;
using namespace rsim;

struct Csc {
    const int* p; const int* i; const double* x; int64_t n, nnz;
    size_t bytes() const { return ((size_t)n + 1) * 4 + (size_t)nnz * 12; }
};

Csc read_csc(const int* p, const int* i, const double* x, const int* nnz, int64_t m, int64_t n, const char* what) {
    if (!p) throw std::invalid_argument(std::string("null col_ptr of ") + what);
    if (!nnz || *nnz < 0) throw std::invalid_argument("nnz must be >= 0");
    if (*nnz > 0 && (!i || !x)) throw std::invalid_argument("null CSC array");
    check_csc_strict(p, i, m, n, *nnz);
    all_finite(x, (size_t)*nnz, what);
    return Csc{p, i, x, n, *nnz};
}

struct DevCsc {
    DevBuf p, i, x;
    void upload_from(const Csc& a, hipStream_t s) {
        upload(p, a.p, (size_t)a.n + 1, s);
        upload(i, a.i, (size_t)a.nnz, s);
        upload(x, a.x, (size_t)a.nnz, s);
    }
};

struct Events {
    hipEvent_t a = nullptr, b = nullptr;
    Events() { HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b)); }
    ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// The rows of the dense entry's chunks: 256 up to 64 chunks, beyond that 64 chunks of whole 256-row blocks.  A function of m alone.
int64_t dense_chunk(int64_t m) {
    const int64_t blocks256 = (m + 255) / 256;
    return 256 * ((blocks256 + 63) / 64);
}

// Minimum-cost assignment of the rows of a (n x mc, n <= mc, row stride `rs`, column stride `cs`) by shortest augmenting paths with
// dual potentials (Jonker-Volgenant form of the Hungarian method), O(n^2 mc).  Rows enter in order and every scan takes the first
// minimum, so equal inputs give equal assignments.  row_of[j]: the row matched to column j, or -1.
void assign_rows(const std::vector<double>& a, int64_t n, int64_t mc, int64_t rs, int64_t cs, std::vector<int>& row_of) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> u(n + 1, 0.0), v(mc + 1, 0.0), minv(mc + 1);
    std::vector<int64_t> p(mc + 1, 0), way(mc + 1, 0);
    std::vector<char> used(mc + 1);
    for (int64_t i = 1; i <= n; ++i) {
        p[0] = i;
        int64_t j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const int64_t i0 = p[j0];
            double delta = inf;
            int64_t j1 = 0;
            for (int64_t j = 1; j <= mc; ++j) {
                if (used[j]) continue;
                const double cur = a[(size_t)((i0 - 1) * rs + (j - 1) * cs)] - u[i0] - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (minv[j] < delta) { delta = minv[j]; j1 = j; }
            }
            for (int64_t j = 0; j <= mc; ++j) {
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int64_t j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0 != 0);
    }
    row_of.assign(mc, -1);
    for (int64_t j = 1; j <= mc; ++j)
        if (p[j] != 0) row_of[j - 1] = (int)(p[j] - 1);
}

}  // namespace

extern "C" int rcppml_gpu_cosine_geometry(int64_t* out) {
    if (!out) return -1;
    out[0] = T;
    out[1] = WAVES;
    out[2] = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) { (void)hipGetLastError(); return 0; }
    const int dev = env_device();
    int cus = 0;
    if (dev >= 0 && dev < count && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) out[2] = cus;
    else (void)hipGetLastError();
    return 0;
}

extern "C" void rcppml_gpu_cosine_sparse_ex(const int* x_col_ptr, const int* x_row_idx, const double* x_values, int* x_nnz,
                                            const int* y_col_ptr, const int* y_row_idx, const double* y_values, int* y_nnz, int* m,
                                            int* nx, int* ny, int* groups, double* out_C, int* out_launches, double* out_ms,
                                            int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !nx) throw std::invalid_argument("null scalar argument");
        const bool self = y_col_ptr == nullptr;
        if (!self && !ny) throw std::invalid_argument("null scalar argument");
        const int64_t M = *m, NX = *nx, NY = self ? NX : *ny;
        if (M < 1 || NX < 1 || NY < 1) throw std::invalid_argument("m, nx and ny must be >= 1");
        if (groups && *groups < 0) throw std::invalid_argument("groups must be >= 0");
        if (!out_C) throw std::invalid_argument("null out_C");
        const Csc X = read_csc(x_col_ptr, x_row_idx, x_values, x_nnz, M, NX, "x");
        const Csc Y = self ? X : read_csc(y_col_ptr, y_row_idx, y_values, y_nnz, M, NY, "y");
        const int64_t ntiles = (NX + T - 1) / T;
        const size_t nC = (size_t)NX * (size_t)NY;
        if ((double)NX * (double)NY * 8.0 > 9.0e18) throw std::invalid_argument("the result does not fit in memory");
        // C, the CSC of X and of X^T (and the transpose's scratch, about as much again), the CSC of Y, the offset table, the norms
        const size_t need = 8 * nC + 3 * X.bytes() + ((size_t)M + 1) * 4 + (self ? 0 : Y.bytes()) +
                            (size_t)(ntiles + 1) * (size_t)M * 4 + (size_t)(NX + NY) * 8 + std::min<size_t>((size_t)256 << 20, (size_t)2048 * (size_t)M) + (1 << 20);
        device_ready(need, "the cosine matrix");
        CtxGuard g(env_device());
        Events ev;
        DevCsc dX, dY;
        DevBuf Tp, Ti, Tx, Ts, Nx, Ny, dC;
        dX.upload_from(X, g.s);
        if (!self) dY.upload_from(Y, g.s);
        HIPCHK(hipStreamSynchronize(g.s));
        HIPCHK(hipEventRecord(ev.a, g.s));
        double* C = dalloc<double>(dC, nC);
        int launches = 0;
        if (X.nnz == 0 || Y.nnz == 0) {
            HIPCHK(hipMemsetAsync(C, 0, nC * 8, g.s));      // every column of one side has zero norm
        } else {
            dalloc<int>(Tp, (size_t)M + 1);
            dalloc<int>(Ti, (size_t)X.nnz);
            dalloc<double>(Tx, (size_t)X.nnz);
            OPCHK(rcppml_hip_transpose_csc(g.c, RCPPML_F64, (int)M, (int)NX, dX.p.as<int>(), dX.i.as<int>(), dX.x.p, Tp.as<int>(),
                                           Ti.as<int>(), Tx.p));
            double* nrmx = dalloc<double>(Nx, (size_t)NX);
            double* nrmy = nrmx;
            hipLaunchKernelGGL(col_norm_kernel, dim3((unsigned)((NX + 255) / 256)), dim3(256), 0, g.s, dX.p.as<int>(),
                               dX.x.as<double>(), NX, nrmx);
            ++launches;
            if (!self) {
                nrmy = dalloc<double>(Ny, (size_t)NY);
                hipLaunchKernelGGL(col_norm_kernel, dim3((unsigned)((NY + 255) / 256)), dim3(256), 0, g.s, dY.p.as<int>(),
                                   dY.x.as<double>(), NY, nrmy);
                ++launches;
            }
            const int64_t nts = (ntiles + 1) * M;
            int* ts = dalloc<int>(Ts, (size_t)nts);
            hipLaunchKernelGGL(tile_offsets_kernel, dim3((unsigned)((nts + 255) / 256)), dim3(256), 0, g.s, Tp.as<int>(), Ti.as<int>(), M,
                               (int)ntiles, ts);
            ++launches;
            HIPCHK(hipGetLastError());
            const int64_t items = NY * ntiles, most = (items + WAVES - 1) / WAVES;
            int64_t grid = (groups && *groups > 0) ? *groups : std::max(1, g.c->num_cu);
            grid = std::max<int64_t>(1, std::min(grid, most));
            const DevCsc& O = self ? dX : dY;
            hipLaunchKernelGGL(cosine_tile_kernel, dim3((unsigned)grid), dim3(NT), 0, g.s, O.p.as<int>(), O.i.as<int>(),
                               O.x.as<double>(), ts, Ti.as<int>(), Tx.as<double>(), nrmx, nrmy, M, NX, NY, (int)ntiles, C);
            ++launches;
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ev.b, g.s));
        HIPCHK(hipStreamSynchronize(g.s));
        float dev_ms = 0.f;
        HIPCHK(hipEventElapsedTime(&dev_ms, ev.a, ev.b));
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipMemcpy(out_C, C, nC * 8, hipMemcpyDeviceToHost));
        const double down_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (out_launches) *out_launches = launches;
        if (out_ms) { out_ms[0] = dev_ms; out_ms[1] = down_ms; }
    });
}

extern "C" void rcppml_gpu_cosine_dense_ex(const double* W, const double* R, int* m, int* kx, int* ky, int* reps, int* method,
                                           double* out, int* out_launches, int* out_status) {
    entry_guard(out_status, [&] {
        if (!m || !kx || !ky || !reps || !method) throw std::invalid_argument("null scalar argument");
        const int64_t M = *m, Q = *reps;
        const int KX = *kx, KY = *ky;
        if (M < 1) throw std::invalid_argument("m must be >= 1");
        if (KX < 1 || KX > DK || KY < 1 || KY > DK) throw std::invalid_argument("kx and ky must be in [1, 128]");
        if (Q < 1) throw std::invalid_argument("reps must be >= 1");
        if (*method != 0 && *method != 1) throw std::invalid_argument("method must be 0 (cosine) or 1 (correlation)");
        if (!W || !R) throw std::invalid_argument("null array");
        if (!out) throw std::invalid_argument("null output");
        const size_t nW = (size_t)Q * (size_t)M * KX, nR = (size_t)M * KY, nOut = (size_t)Q * KX * KY;
        all_finite(W, nW, "W");
        all_finite(R, nR, "R");
        const int64_t chunk = dense_chunk(M), nchunk = (M + chunk - 1) / chunk;
        const size_t ncols = (size_t)Q * KX + KY;
        device_ready((nW + nR + nOut * (size_t)(nchunk + 1) + 2 * ncols) * 8 + 65536, "the dense similarities");
        Stream st;
        DevBuf Wb, Rb, Mb, Nb, Pb, Ob;
        const double* dW = upload<double>(Wb, W, nW, st.s);
        const double* dR = upload<double>(Rb, R, nR, st.s);
        double* mean = dalloc<double>(Mb, ncols);
        double* norm = dalloc<double>(Nb, ncols);
        double* part = dalloc<double>(Pb, nOut * (size_t)nchunk);
        double* dO = dalloc<double>(Ob, nOut);
        hipLaunchKernelGGL(dense_stats_kernel, dim3((unsigned)((ncols + DNT / 64 - 1) / (DNT / 64))), dim3(DNT), 0, st.s, dW, dR, M,
                           (int64_t)Q * KX, (int64_t)KY, *method, mean, norm);
        hipLaunchKernelGGL(dense_partial_kernel, dim3((unsigned)nchunk, (unsigned)Q), dim3(DNT), 0, st.s, dW, dR, M, KX, KY, chunk, mean,
                           Q, part);
        hipLaunchKernelGGL(dense_final_kernel, dim3((unsigned)((nOut + DNT - 1) / DNT)), dim3(DNT), 0, st.s, part, KX, KY, Q, (int)nchunk,
                           norm, dO);
        HIPCHK(hipGetLastError());
        std::vector<double> h(nOut);
        download<double>(h.data(), dO, nOut, st.s);
        std::copy(h.begin(), h.end(), out);
        if (out_launches) *out_launches = 3;
    });
}

extern "C" void rcppml_gpu_bipartite_match_ex(const double* cost, int* nr, int* nc, int* batch, int* out_assignment, double* out_cost,
                                              int* out_status) {
    entry_guard(out_status, [&] {
        if (!nr || !nc || !batch) throw std::invalid_argument("null scalar argument");
        const int64_t NR = *nr, NC = *nc, B = *batch;
        if (NR < 1 || NC < 1) throw std::invalid_argument("nr and nc must be >= 1");
        if (B < 1) throw std::invalid_argument("batch must be >= 1");
        if (!cost) throw std::invalid_argument("null cost");
        if (!out_assignment || !out_cost) throw std::invalid_argument("null output");
        const size_t per = (size_t)NR * (size_t)NC;
        all_finite(cost, per * (size_t)B, "the cost matrix");
        std::vector<int> assign((size_t)B * NR, -1), row_of;
        std::vector<double> total(B, 0.0), a(per);
        for (int64_t b = 0; b < B; ++b) {
            const double* c = cost + (size_t)b * per;
            for (size_t q = 0; q < per; ++q) a[q] = c[q] < 0.0 ? 0.0 : c[q];
            int* as = assign.data() + (size_t)b * NR;
            if (NR <= NC) {
                assign_rows(a, NR, NC, NC, 1, row_of);
                for (int64_t j = 0; j < NC; ++j)
                    if (row_of[j] >= 0) as[row_of[j]] = (int)j;
            } else {
                assign_rows(a, NC, NR, 1, NC, row_of);          // the columns are assigned; a row no column took stays -1
                for (int64_t i = 0; i < NR; ++i) as[i] = row_of[i];
            }
            double s = 0.0;
            for (int64_t i = 0; i < NR; ++i)
                if (as[i] >= 0) s += a[(size_t)(i * NC + as[i])];
            total[b] = s;
        }
        std::copy(assign.begin(), assign.end(), out_assignment);
        std::copy(total.begin(), total.end(), out_cost);
    });
}
