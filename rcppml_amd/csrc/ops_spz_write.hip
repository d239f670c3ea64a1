// ops_spz_write.hip -- StreamPress / SparsePress **v2** `.spz` writer for gfx950: a host CSC -> a file that ops_spz.hip, the
// streamed fits (ops_stream.hip, ops_stream_svd.hip) and the reference's decoder read.  Build-defined entry
// rcppml_gpu_spz_write_ex; it stands for the encoder behind the reference's st_write() (R/streampress.R:69,
// streampress/sparsepress_v2.hpp:480-882) for the lossless value types: uint8 / uint16 / uint32 counts and byte-shuffled fp32 /
// fp64.  Not written: fp16 and quant8 (lossy), row sorting, a transpose section, obs / var tables, v3 files.
//
// Split of the work (kernels_spz_write.hip.h):
//   device  classify ("auto"), symbolise, histogram, normalise, rANS encode, escapes, gather.  The entropy coding runs on the
//           device; there is no host encoder to fall back to.
//   host    the stream table (spz_layout.hpp), two small read-backs -- the check flags with each stream's escape bytes after the
//           symbolise pass, every stream's table and payload size after the encode -- then the layout of the file: header, chunk
//           index, the varint column counts (n bytes or so), the size fields; the data section comes back in one copy.
#include <chrono>
#include <cstdio>
#include "entry_common.hip.h"
#include "kernels_spz_write.hip.h"
using namespace rcppml_spzw;

namespace {

// the values cannot be stored in the integer type asked for: status 2 of the entry, a ValueError of st_write()
struct ValueFitError : std::runtime_error { using std::runtime_error::runtime_error; };

struct StageClock {                     // HIP events between the stages, only when the caller asked for the split
    hipStream_t s; bool on; std::vector<hipEvent_t> ev;
    StageClock(hipStream_t s_, bool on_) : s(s_), on(on_) { mark(); }
    void mark() { if (on) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); ev.push_back(e); HIPCHK(hipEventRecord(e, s)); } }
    void read(double* out, int stages) {
        for (int q = 0; q < stages; ++q) {
            float ms = 0.f;
            if (on && q + 1 < (int)ev.size()) { HIPCHK(hipEventSynchronize(ev[q + 1])); HIPCHK(hipEventElapsedTime(&ms, ev[q], ev[q + 1])); }
            out[q] = ms;
        }
    }
    ~StageClock() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};

struct WriteResult { uint64_t bytes = 0; int vt = 0; uint32_t chunks = 0; };

WriteResult write_spz(const int* col_ptr, const int* row_idx, const double* values, uint64_t nnz, uint32_t m, uint32_t n, const char* path,
                      int vt_req, uint32_t chunk_cols, double* out_ms) {
    const auto wall0 = std::chrono::steady_clock::now();
    // device memory, for the widest type the call can end in: the CSC (16), gaps (4), integer values (4) or planes, one symbol byte
    // per gap and per value byte, 2 bytes of rANS scratch per symbol, escapes (at most 5 per gap; values escape only as integers)
    // and the data section (below the scratch it is gathered from), per nonzero; tables, records and counts per stream
    const uint64_t vb = vt_req == 6 || vt_req < 0 ? 8 : vt_req == 3 ? 4 : 1, chunks = ((uint64_t)n + chunk_cols - 1) / chunk_cols;
    const uint64_t nstreams_max = chunks * (1 + vb);
    device_ready((size_t)(nnz * (16 + 4 + 4 + (1 + vb) * 5 + 10) + ((uint64_t)n + 1) * 4 + nstreams_max * (256 * 16 + W_TABLE + 64 + 40) +
                          (nnz * (1 + vb) / W_HSEG + nstreams_max) * 1032 + ((uint64_t)16 << 20)),
                 "spz_write");
    Stream S;
    hipStream_t s = S.s;
    StageClock clk(s, out_ms != nullptr);
    DevBuf bp, bi, bx, bcls, bsym, bgap, bival, bstr, bseg, besc, bpart, brec, btab, bsz, bscr, beb, bcop, bdata;
    const int* dp = upload(bp, col_ptr, (size_t)n + 1, s);
    const int* di = upload(bi, row_idx, (size_t)nnz, s);
    const double* dx = upload(bx, values, (size_t)nnz, s);
    int vt = vt_req;
    if (vt < 0) {                                                   // "auto": the smallest integer type that holds the data, else fp64
        uint32_t* dcls = zeros<uint32_t>(bcls, 2, s);
        if (nnz) hipLaunchKernelGGL(spzw_classify_kernel, dim3((unsigned)std::min<uint64_t>((nnz + 255) / 256, 4096)), dim3(256), 0, s, dx, (int64_t)nnz, dcls);
        HIPCHK(hipGetLastError());
        uint32_t cls[2];
        download(cls, (const uint32_t*)dcls, 2, s);
        vt = cls[0] ? 6 : cls[1] <= 255u ? 0 : cls[1] <= 65535u ? 1 : 2;
    }
    clk.mark();                                                     // stage 0: upload (+ classify)
    WritePlan P = plan_streams(col_ptr, m, n, nnz, chunk_cols, vt);
    const size_t nstreams = P.streams.size();
    // ---- symbolise
    uint8_t* dsym = dalloc<uint8_t>(bsym, (size_t)P.sym_bytes);
    uint32_t* dgap = dalloc<uint32_t>(bgap, (size_t)nnz);
    uint32_t* dival = dalloc<uint32_t>(bival, P.bpv ? 1 : (size_t)nnz);
    unsigned long long* desc = zeros<unsigned long long>(besc, nstreams + 1, s);
    SymArgs a{dp, di, dx, (int64_t)n, (int)m, chunk_cols, P.spc, vt, vt == 0 ? 255.0 : vt == 1 ? 65535.0 : 4294967295.0, nnz,
              dsym, dgap, dival, desc, (uint64_t)nstreams};
    hipLaunchKernelGGL(spzw_symbolise_kernel, dim3((unsigned)(((uint64_t)n + 3) / 4)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> esc(nstreams + 1);
    download(esc.data(), (const unsigned long long*)desc, nstreams + 1, s);
    clk.mark();                                                     // stage 1: symbolise
    if (esc[nstreams] & WF_ROWS)
        throw std::invalid_argument("malformed CSC: row indices must be strictly increasing within a column and lie in [0, m)");
    if (esc[nstreams] & WF_VALUE)
        throw ValueFitError(std::string("a stored value is not a non-negative integer that fits ") + value_type_name(vt));
    const uint64_t esc_total = place_escapes(P, esc.data());
    // ---- histogram, normalise, encode, escapes
    const WStream* dstr = upload(bstr, P.streams.data(), nstreams, s);
    const WSeg* dseg = upload(bseg, P.segs.data(), P.segs.size(), s);
    uint32_t* dpart = dalloc<uint32_t>(bpart, P.segs.size() * 256);
    uint4* drec = dalloc<uint4>(brec, nstreams * 256);
    uint8_t* dtab = dalloc<uint8_t>(btab, nstreams * W_TABLE);
    uint32_t* dsz = dalloc<uint32_t>(bsz, 2 * nstreams);            // [0, nstreams): table symbols; [nstreams, 2 nstreams): rANS bytes
    uint8_t* dscr = dalloc<uint8_t>(bscr, (size_t)P.scratch_bytes);
    uint8_t* deb = dalloc<uint8_t>(beb, (size_t)esc_total);
    if (!P.segs.empty()) hipLaunchKernelGGL(spzw_hist_kernel, dim3((unsigned)P.segs.size()), dim3(256), 0, s, (const uint8_t*)dsym, dstr, dseg, dpart);
    HIPCHK(hipGetLastError());
    clk.mark();                                                     // stage 2: histogram
    hipLaunchKernelGGL(spzw_normalise_kernel, dim3((unsigned)nstreams), dim3(64), 0, s, dstr, (const uint32_t*)dpart, drec, dtab, dsz);
    HIPCHK(hipGetLastError());
    clk.mark();                                                     // stage 3: normalise
    hipLaunchKernelGGL(spzw_encode_kernel, dim3((unsigned)nstreams), dim3(64), 0, s, (const uint8_t*)dsym, dstr, (const uint4*)drec, dscr, dsz + nstreams);
    HIPCHK(hipGetLastError());
    clk.mark();                                                     // stage 4: rANS encode
    if (esc_total) hipLaunchKernelGGL(spzw_escape_kernel, dim3((unsigned)nstreams), dim3(256), 0, s, (const uint32_t*)dgap, (const uint32_t*)dival, dstr,
                                      (const unsigned long long*)desc, deb);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> sz(2 * nstreams);
    download(sz.data(), (const uint32_t*)dsz, 2 * nstreams, s);      // every stream's sizes, one copy (it also waits for the uploads)
    clk.mark();                                                     // stage 5: escapes
    // ---- assemble
    FileLayout L = layout_data(P, col_ptr, sz.data(), sz.data() + nstreams, esc.data());
    std::vector<uint8_t> file;
    const uint64_t data_off = begin_file(P, L, file);
    if (!L.copies.empty()) {
        const WCopy* dcop = upload(bcop, L.copies.data(), L.copies.size(), s);
        uint8_t* ddata = dalloc<uint8_t>(bdata, (size_t)L.data_size);
        hipLaunchKernelGGL(spzw_gather_kernel, dim3((unsigned)L.copies.size()), dim3(256), 0, s, dcop, (const uint8_t*)dtab, (const uint8_t*)dscr,
                           (const uint8_t*)deb, ddata);
        HIPCHK(hipGetLastError());
        download(file.data() + data_off, (const uint8_t*)ddata, (size_t)L.data_size, s);
    }
    clk.mark();                                                     // stage 6: gather + download
    finish_file(P, L, data_off, file);
    FILE* f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path + " for writing");
    const size_t put = std::fwrite(file.data(), 1, file.size(), f);
    const bool closed = std::fclose(f) == 0;
    if (put != file.size() || !closed) { std::remove(path); throw std::runtime_error(std::string("short write to ") + path); }
    if (out_ms) {
        clk.read(out_ms, 7);
        out_ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    WriteResult R;
    R.bytes = file.size(); R.vt = vt; R.chunks = P.num_chunks;
    return R;
}

}  // namespace

extern "C" void rcppml_gpu_spz_write_ex(const int* col_ptr, const int* row_idx, const double* values, int* nnz, int* m, int* n,
                                        const char* path, int* value_type, int* chunk_cols, int64_t* out_info, double* out_ms,
                                        int* out_status) {
    bool misfit = false;
    entry_guard(out_status, [&] {
        if (!nnz || !m || !n || !value_type || !chunk_cols) throw std::invalid_argument("null scalar argument");
        if (!col_ptr || !path || !out_info || (*nnz > 0 && (!row_idx || !values))) throw std::invalid_argument("null argument");
        if (*m < 1 || *n < 1 || *n > 0x7FFFFFFE) throw std::invalid_argument("m and n must be >= 1 (n at most 2^31 - 2)");
        if (*nnz < 0) throw std::invalid_argument("nnz out of range (at most 2^31 - 1)");
        if (*chunk_cols < 1) throw std::invalid_argument("chunk_cols must be in [1, 2^31 - 1]");
        const int vt = *value_type;
        if (vt == 4 || vt == 5) throw std::invalid_argument("value types float16 and quant8 are lossy: this writer does not produce them");
        if (!(vt == -1 || vt == 0 || vt == 1 || vt == 2 || vt == 3 || vt == 6)) throw std::invalid_argument("unknown value type");
        if (col_ptr[0] != 0 || col_ptr[*n] != *nnz) throw std::invalid_argument("malformed CSC: col_ptr[0] != 0 or col_ptr[n] != nnz");
        for (int j = 0; j < *n; ++j)
            if (col_ptr[j + 1] < col_ptr[j]) throw std::invalid_argument("malformed CSC: col_ptr decreases");
        try {
            const WriteResult R = write_spz(col_ptr, row_idx, values, (uint64_t)*nnz, (uint32_t)*m, (uint32_t)*n, path, vt, (uint32_t)*chunk_cols, out_ms);
            out_info[0] = (int64_t)R.bytes; out_info[1] = R.vt; out_info[2] = R.chunks; out_info[3] = *nnz;
        } catch (const ValueFitError&) { misfit = true; throw; }
    });
    if (misfit) *out_status = 2;
}
