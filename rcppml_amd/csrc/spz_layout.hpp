// spz_layout.hpp -- host-side layout of a StreamPress / SparsePress v2 `.spz` file the device writer (ops_spz_write.hip) produces:
// the table of rANS streams the kernels work through, and, once their sizes are known, where every byte of the file goes.  Plain
// C++17, no HIP, the mirror of spz_parse.hpp: what this header lays out, parse_file() of spz_parse.hpp reads back.
// Format references: streampress/format/header_v2.hpp (header :118-154, chunk descriptor :221-244, footer :252-261, metadata
// :408-431), streampress/sparsepress_v2.hpp:79-172 (gap stream), :179-224 (integer values), :227-304 (byte planes), :598-863 (file).
//
// Streams.  A chunk of `chunk_cols` columns has `spc` streams: its gaps, then either its integer values (value types 0..2) or the
// bpv byte planes of its floats (3: fp32, 6: fp64).  Stream c * spc + q belongs to chunk c; a chunk without nonzeros keeps its
// slots with count 0, which every kernel skips.
//
// A chunk without nonzeros still gets a well-formed count section, [u32 size][one zero byte per column]: the reference encoder
// omits the size there (sparsepress_v2.hpp:94) and its decoder then reads whatever bytes follow as counts (:991-1003); with the
// section present every decoder reads zeros and nothing after them.
#pragma once
#include <stdexcept>
#include <string>
#include "spz_parse.hpp"

namespace rcppml_spz {

constexpr uint32_t W_HSEG = 65536;          // symbols per histogram workgroup
constexpr uint32_t W_PIECE = 65536;         // bytes per workgroup of the gather kernel
constexpr uint32_t W_TABLE = 514;           // a serialized table of 256 symbols (rans.hpp:138-149)

struct WStream {                            // one rANS stream of the writer
    uint64_t sym_off;                       // its symbols (one byte each, contiguous) in the symbol array
    uint64_t src_off;                       // its u32 source elements (gaps / integer values), which the escapes are taken from
    uint64_t scratch_off;                   // its 2 * count + 4 bytes of rANS scratch, filled from the end
    uint64_t esc_off;                       // its varint escapes in the escape scratch
    uint32_t count, kind, seg0, nseg;       // kind: JOB_GAPS / JOB_INT / JOB_PLANE; histogram segments [seg0, seg0 + nseg)
};
struct WSeg { uint32_t stream, start; };    // W_HSEG symbols of a stream from `start`
struct WCopy { uint64_t src, dst; uint32_t len, which; };   // which: 0 tables, 1 rANS scratch, 2 escape scratch; dst in the data section

inline uint32_t value_bytes(int vt) { return vt == 3 ? 4u : vt == 6 ? 8u : 0u; }
inline const char* value_type_name(int vt) {
    static const char* names[] = {"uint8", "uint16", "uint32", "float32", "float16", "quant8", "float64"};
    return vt >= 0 && vt <= 6 ? names[vt] : "unknown";
}

struct WritePlan {
    uint32_t m = 0, n = 0, chunk_cols = 0, num_chunks = 0, bpv = 0, spc = 0;
    uint64_t nnz = 0, sym_bytes = 0, scratch_bytes = 0;
    int vt = 0;
    std::vector<WStream> streams;
    std::vector<WSeg> segs;
};

// col_ptr is checked by the caller (starts at 0, never decreases, ends at nnz)
inline WritePlan plan_streams(const int* col_ptr, uint32_t m, uint32_t n, uint64_t nnz, uint32_t chunk_cols, int vt) {
    WritePlan P;
    P.m = m; P.n = n; P.nnz = nnz; P.chunk_cols = chunk_cols; P.vt = vt;
    P.num_chunks = (uint32_t)(((uint64_t)n + chunk_cols - 1) / chunk_cols);
    P.bpv = value_bytes(vt);
    P.spc = 1 + (P.bpv ? P.bpv : 1);
    P.sym_bytes = nnz * (1 + (uint64_t)(P.bpv ? P.bpv : 1));
    P.streams.resize((size_t)P.num_chunks * P.spc);
    for (uint32_t c = 0; c < P.num_chunks; ++c) {
        const uint64_t j0 = (uint64_t)c * chunk_cols, j1 = std::min<uint64_t>(j0 + chunk_cols, n);
        const uint64_t o = (uint64_t)col_ptr[j0], cnt = (uint64_t)col_ptr[j1] - o;
        for (uint32_t q = 0; q < P.spc; ++q) {
            WStream& s = P.streams[(size_t)c * P.spc + q];
            s.count = (uint32_t)cnt;
            s.src_off = o;
            if (q == 0) { s.kind = JOB_GAPS; s.sym_off = o; }
            else if (!P.bpv) { s.kind = JOB_INT; s.sym_off = nnz + o; }
            else { s.kind = JOB_PLANE; s.sym_off = nnz + o * P.bpv + (uint64_t)(q - 1) * cnt; }   // plane-major inside the chunk
            s.scratch_off = P.scratch_bytes;
            if (cnt) P.scratch_bytes += 2 * cnt + 4;
            s.seg0 = (uint32_t)P.segs.size();
            for (uint64_t st = 0; st < cnt; st += W_HSEG) P.segs.push_back(WSeg{(uint32_t)((size_t)c * P.spc + q), (uint32_t)st});
            s.nseg = (uint32_t)P.segs.size() - s.seg0;
        }
    }
    return P;
}

// escape offsets from the sizes the symbolise kernel counted; returns their sum
inline uint64_t place_escapes(WritePlan& P, const unsigned long long* esc_bytes) {
    uint64_t off = 0;
    for (size_t s = 0; s < P.streams.size(); ++s) { P.streams[s].esc_off = off; off += esc_bytes[s]; }
    return off;
}

// CRC-32 (ISO 3309, reflected polynomial 0xEDB88320) of the file before its footer, as format/checksum.hpp computes it
inline uint32_t crc32(const uint8_t* p, size_t len) {
    static uint32_t table[256];
    static bool ready = false;
    if (!ready) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int b = 0; b < 8; ++b) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        ready = true;
    }
    uint32_t crc = 0xFFFFFFFFu;
    for (size_t i = 0; i < len; ++i) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return crc ^ 0xFFFFFFFFu;
}

struct FileLayout {
    std::vector<SpzChunk> chunks;
    std::vector<WCopy> copies;                      // device bytes -> data section, in pieces of at most W_PIECE
    struct Lit { uint64_t dst; size_t off, len; };  // host-built bytes (sizes, count sections) -> data section
    std::vector<Lit> lits;
    std::vector<uint8_t> lit;
    uint64_t data_size = 0;

    void put(const void* p, size_t len) {
        lits.push_back(Lit{data_size, lit.size(), len});
        lit.insert(lit.end(), static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + len);
        data_size += len;
    }
    void put32(uint32_t v) { put(&v, 4); }
    void copy(uint32_t which, uint64_t src, uint64_t len) {
        for (uint64_t o = 0; o < len; o += W_PIECE) copies.push_back(WCopy{src + o, data_size + o, (uint32_t)std::min<uint64_t>(W_PIECE, len - o), which});
        data_size += len;
    }
};

// ns[s]: symbols of stream s's table, enc[s]: its rANS bytes (the LAST enc[s] bytes of its scratch region), esc[s]: its escape bytes
inline FileLayout layout_data(const WritePlan& P, const int* col_ptr, const uint32_t* ns, const uint32_t* enc, const unsigned long long* esc) {
    FileLayout L;
    L.chunks.resize(P.num_chunks);
    std::vector<uint8_t> cc;
    auto rans_block = [&](size_t s, bool escapes) {
        const WStream& w = P.streams[s];
        L.copy(0, (uint64_t)s * W_TABLE, 2 + 2ull * ns[s]);
        L.put32(enc[s]);
        L.copy(1, w.scratch_off + (2ull * w.count + 4 - enc[s]), enc[s]);
        if (escapes) {
            if (esc[s] > 0xFFFFFFFFull) throw std::runtime_error("spz_write: a chunk's escape section exceeds 4 GiB; use a smaller chunk_cols");
            L.put32((uint32_t)esc[s]);
            L.copy(2, w.esc_off, esc[s]);
        }
    };
    for (uint32_t c = 0; c < P.num_chunks; ++c) {
        SpzChunk& d = L.chunks[c];
        std::memset(&d, 0, sizeof d);
        const size_t s0 = (size_t)c * P.spc;
        const uint64_t j0 = (uint64_t)c * P.chunk_cols, j1 = std::min<uint64_t>(j0 + P.chunk_cols, P.n);
        d.col_start = (uint32_t)j0; d.num_cols = (uint32_t)(j1 - j0); d.nnz = P.streams[s0].count;
        cc.clear();
        for (uint64_t j = j0; j < j1; ++j) {                                 // varint column counts (codec/varint.hpp)
            uint32_t v = (uint32_t)(col_ptr[j + 1] - col_ptr[j]);
            while (v >= 0x80) { cc.push_back((uint8_t)(v | 0x80)); v >>= 7; }
            cc.push_back((uint8_t)v);
        }
        const uint64_t g0 = L.data_size;
        L.put32((uint32_t)cc.size());
        L.put(cc.data(), cc.size());
        if (d.nnz) rans_block(s0, true);
        const uint64_t v0 = L.data_size;
        if (d.nnz) {
            if (!P.bpv) rans_block(s0 + 1, true);
            else {
                const uint8_t planes = (uint8_t)P.bpv;
                L.put(&planes, 1);
                for (uint32_t q = 0; q < P.bpv; ++q) { L.put32(2 + 2 * ns[s0 + 1 + q]); rans_block(s0 + 1 + q, false); }
            }
        }
        if (L.data_size > 0xFFFFFFFFull) throw std::runtime_error("spz_write: the data section exceeds the format's 4 GiB of stream offsets");
        d.stream_offset[0] = (uint32_t)g0; d.stream_size[0] = (uint32_t)(v0 - g0);
        d.stream_offset[1] = (uint32_t)v0; d.stream_size[1] = (uint32_t)(L.data_size - v0);
        d.decoded_gap_bytes = d.nnz * 4u;
        d.decoded_value_bytes = d.nnz * (P.vt == 0 ? 1u : P.vt == 1 ? 2u : P.vt == 6 ? 8u : 4u);
    }
    return L;
}

// Sizes `file` and writes everything but the device-made bytes of the data section: header, chunk index, the host-built pieces.
// Returns the offset of the data section.  finish_file() follows once the data section has been copied in (the pieces again,
// since the device copy covers the whole section), and appends the empty metadata section and the footer.
inline uint64_t begin_file(const WritePlan& P, const FileLayout& L, std::vector<uint8_t>& file) {
    SpzHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, "SPRZ", 4);
    h.version = 2; h.header_size = 128;
    h.m = P.m; h.n = P.n; h.nnz = P.nnz; h.chunk_cols = P.chunk_cols; h.num_chunks = P.num_chunks;
    h.table_log = 11; h.value_type = (uint8_t)P.vt; h.compression_level = 1;
    h.chunk_index_offset = 128;
    h.tables_offset = h.data_offset = 128 + (uint64_t)P.num_chunks * 48;
    h.metadata_offset = h.data_offset + L.data_size;
    h.density = (float)P.nnz / ((float)P.m * (float)P.n);
    file.assign((size_t)(h.metadata_offset + 4 + 16), 0);
    std::memcpy(file.data(), &h, 128);
    if (P.num_chunks) std::memcpy(file.data() + 128, L.chunks.data(), (size_t)P.num_chunks * 48);
    return h.data_offset;
}
inline void finish_file(const WritePlan& P, const FileLayout& L, uint64_t data_offset, std::vector<uint8_t>& file) {
    for (const FileLayout::Lit& q : L.lits) std::memcpy(file.data() + data_offset + q.dst, L.lit.data() + q.off, q.len);
    uint8_t* tail = file.data() + data_offset + L.data_size;                // metadata: u32 entry count = 0
    std::memset(tail, 0, 4);
    const uint32_t foot[3] = {4u, crc32(file.data(), file.size() - 16), P.num_chunks};   // metadata size, CRC, chunks
    std::memcpy(tail + 4, foot, 12);
    std::memcpy(tail + 16, "SPEN", 4);
}

}  // namespace rcppml_spz
