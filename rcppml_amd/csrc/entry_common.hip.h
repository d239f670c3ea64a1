// entry_common.hip.h -- the host-side scaffold of the build-defined entry files (ops_cluster, ops_svd, ops_assess, ops_distribution,
// ops_consensus, ops_refine, ops_zi): the guard around an extern "C" body, the device check, the argument checks every entry
// repeats (finite values, the two CSC checks), a stream guard, the DevBuf helpers and the reference's SplitMix64 draws.  Host code
// only, no kernels and no translation unit of its own.  An entry file keeps what is specific to it: its argument structs, engines,
// launches and host algorithms.
#pragma once
#include "plugin_common.hip.h"

#include <climits>

namespace rcppml_plugin {

// The body of an extern "C" entry: *out_status = 0 when `body` returns, -1 with the reason in rcppml_err() when it throws (never
// across the C ABI).  A null out_status returns at once.
template <class Body> void entry_guard(int* out_status, Body body) {
    if (!out_status) return;
    try {
        rcppml_err().clear();
        body();
        *out_status = 0;
    } catch (const std::exception& e) {
        rcppml_err() = e.what();
        *out_status = -1;
    } catch (...) {
        rcppml_err() = "unknown error";
        *out_status = -1;
    }
}

// device present, device selected (RCPPML_GPU_DEVICE), `need` bytes free; allocates and launches nothing
inline void device_ready(size_t need, const char* what = "the call") {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        throw std::runtime_error("no HIP device");
    }
    const int dev = env_device();
    if (dev < 0 || dev >= count) throw std::runtime_error("RCPPML_GPU_DEVICE names no device");
    HIPCHK(hipSetDevice(dev));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b)
        throw std::runtime_error(std::string(what) + " needs " + std::to_string(need) + " bytes of device memory, " +
                                 std::to_string(free_b) + " are free");
}

inline void all_finite(const double* v, size_t count, const char* what) {
    for (size_t q = 0; q < count; ++q)
        if (!std::isfinite(v[q])) throw std::invalid_argument(std::string(what) + " holds a non-finite value");
}

// The two CSC checks; finite values are the caller's to check.
// strict: rows strictly increasing within a column (the dgCMatrix invariant).  Null pointers and the range of nnz are checked by
// the caller first (they differ by entry).
inline void check_csc_strict(const int* col_ptr, const int* row_idx, int64_t m, int64_t n, int64_t nnz) {
    if (col_ptr[0] != 0 || col_ptr[n] != nnz) throw std::invalid_argument("malformed CSC: col_ptr[0] != 0 or col_ptr[n] != nnz");
    for (int64_t j = 0; j < n; ++j) {
        if (col_ptr[j + 1] < col_ptr[j]) throw std::invalid_argument("malformed CSC: col_ptr decreases");
        for (int e = col_ptr[j]; e < col_ptr[j + 1]; ++e) {
            if (row_idx[e] < 0 || row_idx[e] >= m) throw std::invalid_argument("malformed CSC: a row index outside [0, m)");
            if (e > col_ptr[j] && row_idx[e] <= row_idx[e - 1])
                throw std::invalid_argument("malformed CSC: row indices not strictly increasing within a column");
        }
    }
}
// lenient: any row order within a column (the reference plugin's entries take what R hands over), nnz below INT_MAX
inline void check_csc_lenient(const int* col_ptr, const int* row_idx, const double* values, int m, int n, int64_t nnz) {
    if (nnz < 0 || nnz >= INT_MAX) throw std::invalid_argument("nnz out of range");
    if (!col_ptr || (nnz > 0 && (!row_idx || !values))) throw std::invalid_argument("null CSC array");
    if (col_ptr[0] != 0 || (int64_t)col_ptr[n] != nnz) throw std::invalid_argument("col_ptr must start at 0 and end at nnz");
    for (int j = 0; j < n; ++j)
        if (col_ptr[j + 1] < col_ptr[j]) throw std::invalid_argument("col_ptr must be non-decreasing");
    for (int64_t e = 0; e < nnz; ++e)
        if (row_idx[e] < 0 || row_idx[e] >= m) throw std::invalid_argument("row index out of range");
}

// a non-blocking stream on the current device
struct Stream {
    hipStream_t s = nullptr;
    Stream() { HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    void sync() { HIPCHK(hipStreamSynchronize(s)); }
};

// DevBuf helpers.  An empty count allocates one element and copies nothing.  upload is asynchronous: the host source must outlive
// the copy (synchronise the stream before it goes away); download waits for the stream.
template <class T> T* dalloc(DevBuf& b, size_t count) {
    b.alloc(std::max<size_t>(count, 1) * sizeof(T));
    return b.as<T>();
}
// grow-only: keeps the allocation when it is large enough
template <class T> T* grow(DevBuf& b, size_t count) {
    if (b.bytes < count * sizeof(T) || !b.p) b.alloc(count * sizeof(T));
    return b.as<T>();
}
template <class T> T* upload(DevBuf& b, const T* h, size_t count, hipStream_t s) {
    T* p = dalloc<T>(b, count);
    if (count) HIPCHK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
    return p;
}
template <class T> T* zeros(DevBuf& b, size_t count, hipStream_t s) {
    T* p = dalloc<T>(b, count);
    HIPCHK(hipMemsetAsync(p, 0, std::max<size_t>(count, 1) * sizeof(T), s));
    return p;
}
template <class T> void download(T* h, const T* d, size_t count, hipStream_t s) {
    if (count) HIPCHK(hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
}

// SplitMix64 uniform<S>() draws (rng/rng.hpp:89-104): draw `off` .. off + count - 1 of the stream of `seed`
template <class S> std::vector<S> splitmix(uint64_t seed, uint64_t off, size_t count) {
    constexpr uint64_t golden = 0x9e3779b97f4a7c15ull;
    std::vector<S> out(count);
    uint64_t state = seed + off * golden;
    for (auto& x : out) {
        state += golden;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z = z ^ (z >> 31);
        x = static_cast<S>(z) / static_cast<S>(UINT64_MAX);
    }
    return out;
}

}  // namespace rcppml_plugin
