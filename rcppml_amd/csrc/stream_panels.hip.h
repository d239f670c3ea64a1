// stream_panels.hip.h -- the panel source of the streamed fits (ops_stream.hip, ops_stream_svd.hip): a matrix given
// as a host CSC or as the path of an .spz file, cut into column panels that pass through one device buffer.  PanelSource opens and
// checks the matrix and plans the panels on the host; PanelBuffer<T> is the device buffer and makes one panel resident, uploaded
// from the host CSC or decoded from the file's chunks (rcppml_spz_decode_columns, ops_spz.hip).  Host code only.
#pragma once
#include "entry_common.hip.h"
#include "spz_parse.hpp"

#include <cstdio>

// ops_spz.hip: whole chunks of a parsed .spz file into device arrays
void rcppml_spz_decode_columns(rcppml_hip_ctx* c, const uint8_t* data, const rcppml_spz::SpzParsed& P, int64_t col0, int64_t col1,
                               int* d_col_ptr, int* d_row_idx, double* d_values, int check_rows_below);

namespace rcppml_plugin {

inline std::vector<uint8_t> read_file(const char* path) {
    struct File { FILE* f; ~File() { if (f) std::fclose(f); } } file{std::fopen(path, "rb")};
    if (!file.f) throw std::invalid_argument(std::string("cannot open ") + path);
    long fsz = -1;
    if (std::fseek(file.f, 0, SEEK_END) == 0) fsz = std::ftell(file.f);
    if (fsz < 0 || std::fseek(file.f, 0, SEEK_SET) != 0) throw std::invalid_argument(std::string("cannot size ") + path);
    std::vector<uint8_t> bytes((size_t)fsz);
    if (fsz && std::fread(bytes.data(), 1, (size_t)fsz, file.f) != (size_t)fsz) throw std::invalid_argument(std::string("short read of ") + path);
    return bytes;
}

struct PanelSource {
    const int* p = nullptr; const int* i = nullptr; const double* x = nullptr;      // a host CSC ...
    std::vector<uint8_t> bytes; rcppml_spz::SpzParsed parsed; bool spz = false;      // ... or the bytes of an .spz file and their parse
    std::vector<int64_t> chunk_start;        // .spz: the first column of every chunk, then n
    int64_t m = 0, n = 0, total_nnz = 0;
    std::vector<int64_t> pb;                 // panel q holds columns pb[q] .. pb[q + 1]
    int64_t pc = 0, max_nnz = 0;             // the widest panel's columns, the fullest panel's nonzeros
    const int* colptr() const { return spz ? parsed.col_ptr.data() : p; }
    int64_t panels() const { return (int64_t)pb.size() - 1; }

    // a StreamPress v2 file of shape m x n, not row-sorted, its chunks contiguous in column order
    void open_spz(const char* path, int64_t m_, int64_t n_) {
        m = m_; n = n_; spz = true;
        bytes = read_file(path);
        try { parsed = rcppml_spz::parse_file(bytes.data(), bytes.size()); }
        catch (const rcppml_spz::ParseError& e) { throw std::invalid_argument(std::string("data = an .spz path: ") + e.what); }
        const rcppml_spz::SpzHeader& h = parsed.h;
        if ((int64_t)h.m != m || (int64_t)h.n != n) throw std::invalid_argument("data = an .spz path: the file's shape is not m x n");
        if (!parsed.row_perm.empty()) throw std::invalid_argument("data = an .spz path: a row-sorted file (stored row permutation) does not keep rows ascending within a column");
        for (int64_t j = 0; j < n; ++j)
            if (parsed.col_ptr[j] < 0 || parsed.col_ptr[j] > parsed.col_ptr[j + 1]) throw std::invalid_argument("data = an .spz path: column pointers not monotone");
        if (parsed.col_ptr[0] != 0 || (uint64_t)parsed.col_ptr[n] != h.nnz) throw std::invalid_argument("data = an .spz path: column pointers do not span the nonzeros");
        std::vector<rcppml_spz::SpzChunk> ch(h.num_chunks);
        if (h.num_chunks) std::memcpy(ch.data(), bytes.data() + h.chunk_index_offset, (size_t)h.num_chunks * 48);
        int64_t next = 0;
        for (const auto& cdesc : ch) {
            if ((int64_t)cdesc.col_start != next) throw std::invalid_argument("data = an .spz path: chunks are not contiguous in column order");
            chunk_start.push_back(next);
            next += cdesc.num_cols;
        }
        if (next != n) throw std::invalid_argument("data = an .spz path: chunks do not cover the columns");
        chunk_start.push_back(n);
        total_nnz = (int64_t)h.nnz;
    }
    // a host CSC of shape m x n, rows strictly increasing within a column, finite values
    void open_csc(const int* col_ptr, const int* row_idx, const double* values, const int* nnz, int64_t m_, int64_t n_) {
        m = m_; n = n_;
        if (!nnz || *nnz < 0) throw std::invalid_argument("nnz must be >= 0");
        if (!col_ptr || (*nnz > 0 && (!row_idx || !values))) throw std::invalid_argument("null CSC array");
        check_csc_strict(col_ptr, row_idx, m, n, *nnz);
        all_finite(values, (size_t)*nnz, "the matrix");
        p = col_ptr; i = row_idx; x = values;
        total_nnz = *nnz;
    }
    // The panels: panel_cols columns each; from an .spz file whole chunks, panel_cols rounded up to them.  panel_cols = 0: about 64 MiB
    // of CSC at the matrix's mean column size, in whole multiples of 256 columns, and no wider than `cap` columns (the caller's
    // range table).  An explicit width above cap is the caller's to refuse (pc holds the widest panel).
    void plan(int64_t panel_cols, int64_t cap) {
        int64_t w = panel_cols;
        if (w == 0) {
            const double col_bytes = 4.0 + 12.0 * (double)total_nnz / (double)n;
            w = std::max<int64_t>(256, (int64_t)(67108864.0 / col_bytes) / 256 * 256);
            w = std::min(w, std::max<int64_t>(1, spz ? cap : (cap >= 256 ? cap / 256 * 256 : cap)));
        }
        if (spz && parsed.h.chunk_cols > 0) w = (w + parsed.h.chunk_cols - 1) / parsed.h.chunk_cols * parsed.h.chunk_cols;
        w = std::min(w, n);
        pb.assign(1, 0);
        if (spz) {
            for (size_t q = 1; q < chunk_start.size(); ++q)
                if (q + 1 == chunk_start.size() || chunk_start[q + 1] - pb.back() > w) pb.push_back(chunk_start[q]);
        } else {
            for (int64_t j = w; j < n; j += w) pb.push_back(j);
            pb.push_back(n);
        }
        const int* cp = colptr();
        pc = 0; max_nnz = 0;
        for (size_t q = 0; q + 1 < pb.size(); ++q) {
            pc = std::max(pc, pb[q + 1] - pb[q]);
            max_nnz = std::max<int64_t>(max_nnz, cp[pb[q + 1]] - cp[pb[q]]);
        }
    }
    // device bytes of the panel buffer: column pointers, rows, values in the fit's precision and, for fp32, the doubles they are cast from
    size_t buffer_bytes(size_t elem) const { return ((size_t)pc + 1) * 4 + (size_t)max_nnz * (4 + elem + (elem == 4 ? 8 : 0)); }
    // .spz: what the decoder allocates beside the buffer for one panel, generously
    size_t decode_bytes() const { return spz ? bytes.size() / (size_t)panels() * 2 + (size_t)max_nnz * 8 : 0; }
};

// One panel buffer: everything runs on one stream, so a second one would overlap nothing.
template <class T> struct PanelBuffer {
    static constexpr bool f32 = std::is_same<T, float>::value;
    const PanelSource& S;
    rcppml_hip_ctx* c;
    hipStream_t s;
    DevBuf bp, bi, bx, bx64;
    std::vector<int> hp;                     // host CSC: every panel's column pointers, rebased to its first nonzero
    PanelBuffer(const PanelSource& S_, rcppml_hip_ctx* c_, hipStream_t s_) : S(S_), c(c_), s(s_) {
        if (!S.spz) {
            const int* cp = S.colptr();
            hp.resize((size_t)(S.n + S.panels()));
            for (int64_t q = 0; q < S.panels(); ++q)
                for (int64_t j = S.pb[q]; j <= S.pb[q + 1]; ++j) hp[(size_t)(j + q)] = cp[j] - cp[S.pb[q]];
        }
        dalloc<int>(bp, (size_t)S.pc + 1);
        dalloc<int>(bi, (size_t)S.max_nnz);
        dalloc<T>(bx, (size_t)S.max_nnz);
        if (f32) dalloc<double>(bx64, (size_t)S.max_nnz);      // the boundary's doubles, cast on the device
    }
    const int* cp() const { return bp.as<int>(); }
    const int* ri() const { return bi.as<int>(); }
    const T* ax() const { return bx.as<T>(); }
    // panel q resident in the buffer; check_rows: the decoded rows are checked against m (the first visit of an .spz panel)
    void load(int64_t q, bool check_rows) {
        const int* hcp = S.colptr();
        const int64_t j0 = S.pb[q], j1 = S.pb[q + 1], e0 = hcp[j0], pn = hcp[j1] - e0;
        double* const x64 = f32 ? bx64.as<double>() : reinterpret_cast<double*>(bx.p);
        if (S.spz) {
            rcppml_spz_decode_columns(c, S.bytes.data(), S.parsed, j0, j1, bp.as<int>(), bi.as<int>(), x64, check_rows ? (int)S.m : 0);
        } else {
            HIPCHK(hipMemcpyAsync(bp.p, hp.data() + j0 + q, (size_t)(j1 - j0 + 1) * 4, hipMemcpyHostToDevice, s));
            if (pn > 0) {
                HIPCHK(hipMemcpyAsync(bi.p, S.i + e0, (size_t)pn * 4, hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(x64, S.x + e0, (size_t)pn * 8, hipMemcpyHostToDevice, s));
            }
        }
        if (f32 && pn > 0) OPCHK(rcppml_hip_cast(c, RCPPML_F64, x64, RCPPML_F32, bx.p, pn));
    }
};

}  // namespace rcppml_plugin
