// kernels_spz_write.hip.h -- the device half of the StreamPress v2 writer (ops_spz_write.hip): CSC arrays -> the entropy-coded
// bytes of every rANS stream of the file.  The mirror of the reader's kernels (ops_spz.hip): there one wavefront decodes a stream
// on a wave-uniform state; here one wavefront encodes it, with a histogram and a normalisation stage in front.
//
//   spzw_classify_kernel    ("auto" only) are all values non-negative integers below 2^32, and their maximum
//   spzw_symbolise_kernel   one wavefront per column: rows -> gaps, values -> symbols (min(v, 255), or the byte planes of a float,
//                           plane-major inside the chunk so that every stream reads contiguous bytes); checks rows and values;
//                           counts each stream's escape bytes
//   spzw_hist_kernel        one workgroup per W_HSEG symbols of a stream: 256 integer counts in LDS, one copy per wavefront
//   spzw_normalise_kernel   one wavefront per stream: counts -> 14-bit frequencies, the serialized table, the encode records
//   spzw_encode_kernel      one wavefront per stream: the rANS recurrence, last symbol first
//   spzw_escape_kernel      one workgroup per stream: varints of the escaped elements, placed by prefix sums, forward order
//   spzw_gather_kernel      tables, rANS bytes and escapes -> their places in the file's data section
// Every count is an integer and every sum has one order: two runs write the same bytes.
#pragma once
#include "common.hip.h"
#include "spz_layout.hpp"

namespace rcppml_spzw {
using namespace rcppml_spz;

constexpr int W_PROB_BITS = 14;
constexpr uint32_t W_SCALE = 1u << W_PROB_BITS;
constexpr uint32_t W_L = 1u << 23;              // lower bound of the state (rans.hpp:173)
constexpr int W_B = 2048;                       // symbols per staging block of the encoder
constexpr int W_OB = 2 * W_B + 4;               // bytes a block can emit: two per symbol, + the final state
enum { WF_ROWS = 1, WF_VALUE = 2 };

__device__ __forceinline__ uint32_t w_rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t w_varint_len(uint32_t v) { return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u; }
// a value an integer type of maximum `vmax` stores exactly: not negative (-0.0 has a sign to lose), whole, in range; NaN fails
__device__ __forceinline__ bool w_fits(double v, double vmax) { return __double_as_longlong(v) >= 0 && v <= vmax && v == floor(v); }

// out[0] |= 1 when a value is no non-negative integer below 2^32; out[1] = max of those that are
__global__ __launch_bounds__(256) void spzw_classify_kernel(const double* __restrict__ values, int64_t nnz, uint32_t* __restrict__ out) {
    uint32_t bad = 0, mx = 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * 256) {
        const double v = values[t];
        if (w_fits(v, 4294967295.0)) mx = max(mx, (uint32_t)v); else bad = 1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { bad |= __shfl_xor(bad, off, 64); mx = max(mx, __shfl_xor(mx, off, 64)); }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(out, 1u);
        atomicMax(out + 1, mx);
    }
}

struct SymArgs {
    const int* col_ptr; const int* rows; const double* values;
    int64_t n; int m; uint32_t chunk_cols, spc; int vt; double vmax; uint64_t nnz;
    uint8_t* syms; uint32_t* gaps; uint32_t* ivals;
    unsigned long long* esc_bytes;      // per stream; the word after the last stream collects the WF_* flags
    uint64_t nstreams;
};

// One wavefront per column (the inverse of spz_rows_kernel): gap_0 = row_0, gap_t = row_t - row_{t-1} - 1.  A row that does not
// ascend or lies outside [0, m), or a value the integer type cannot hold, raises a flag and is encoded as 0: nothing faults, the
// host reads the flags before it goes on.
__global__ __launch_bounds__(256) void spzw_symbolise_kernel(SymArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + wave;
    if (j >= a.n) return;
    const int s = a.col_ptr[j], e = a.col_ptr[j + 1];
    const int64_t c = j / a.chunk_cols, j0 = c * (int64_t)a.chunk_cols, j1 = min(j0 + (int64_t)a.chunk_cols, a.n);
    const uint64_t oc = (uint64_t)a.col_ptr[j0], nc = (uint64_t)a.col_ptr[j1] - oc;
    const uint32_t bpv = a.vt == 3 ? 4u : a.vt == 6 ? 8u : 0u;
    uint32_t bad = 0;
    unsigned long long eg = 0, ev = 0;
    for (int t0 = s; t0 < e; t0 += 64) {
        const int t = t0 + lane;
        if (t >= e) break;
        const int r = a.rows[t], prev = t > s ? a.rows[t - 1] : -1;
        uint32_t gap = 0;
        if (r < 0 || r >= a.m || r <= prev) bad |= WF_ROWS; else gap = (uint32_t)(r - prev - 1);
        a.gaps[t] = gap;
        a.syms[t] = (uint8_t)min(gap, 255u);
        if (gap >= 255u) eg += w_varint_len(gap);
        const double v = a.values[t];
        if (bpv == 0) {
            uint32_t iv = 0;
            if (w_fits(v, a.vmax)) iv = (uint32_t)v; else bad |= WF_VALUE;
            a.ivals[t] = iv;
            a.syms[a.nnz + t] = (uint8_t)min(iv, 255u);
            if (iv >= 255u) ev += w_varint_len(iv);
        } else {
            uint8_t* pl = a.syms + a.nnz + oc * bpv + ((uint64_t)t - oc);
            if (bpv == 4) {
                const uint32_t b = __float_as_uint((float)v);
#pragma unroll
                for (int q = 0; q < 4; ++q) pl[q * nc] = (uint8_t)(b >> (8 * q));
            } else {
                const uint64_t b = (uint64_t)__double_as_longlong(v);
#pragma unroll
                for (int q = 0; q < 8; ++q) pl[q * nc] = (uint8_t)(b >> (8 * q));
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bad |= __shfl_xor(bad, off, 64);
        eg += __shfl_xor(eg, off, 64);
        ev += __shfl_xor(ev, off, 64);
    }
    if (lane == 0) {                    // integer atomics: the sums do not depend on their order
        if (eg) atomicAdd(a.esc_bytes + (uint64_t)c * a.spc, eg);
        if (ev) atomicAdd(a.esc_bytes + (uint64_t)c * a.spc + 1, ev);
        if (bad) atomicOr(a.esc_bytes + a.nstreams, (unsigned long long)bad);
    }
}

// 256 counts of W_HSEG symbols: each wavefront counts into its own copy (a quarter of the collisions of a skewed stream), the copies
// are added in wavefront order
__global__ __launch_bounds__(256) void spzw_hist_kernel(const uint8_t* __restrict__ syms, const WStream* __restrict__ streams,
                                                        const WSeg* __restrict__ segs, uint32_t* __restrict__ partial) {
    __shared__ uint32_t h[4][256];
    const WSeg sg = segs[blockIdx.x];
    const WStream st = streams[sg.stream];
    const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < 4; ++w) h[w][tid] = 0;
    __syncthreads();
    const uint32_t len = min(W_HSEG, st.count - sg.start);
    const uint8_t* p = syms + st.sym_off + sg.start;
    for (uint32_t i = tid; i < len; i += 256) atomicAdd(&h[wave][p[i]], 1u);
    __syncthreads();
    partial[(size_t)blockIdx.x * 256 + tid] = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
}

// One wavefront per stream, lane L owning symbols 4 L .. 4 L + 3.  The rule (integers only; NOT the reference's, whose table comes
// from double arithmetic and an unstable sort, rans.hpp:55-125 -- any table that sums to 2^14 decodes, it is stored in the file):
//   every present symbol starts at 1; the other 2^14 - present slots are shared out in proportion, rounded down,
//   f = 1 + floor(count * (2^14 - present) / total); what the rounding left over (fewer than `present` slots) goes one each to the
//   symbols with the largest remainders, the lower symbol first among equals.
// Absent symbols get 0, a lone symbol 2^14, the sum is 2^14 exactly.  The encode record of a symbol is {x_max, rcp, freq | k << 16,
// cum}: x_max = ((2^23 >> 14) << 8) * freq (rans.hpp:187), and floor(x / freq) = (x * rcp) >> k for every x < 2^31, with
// k = 31 + ceil(log2 freq) and rcp = ceil(2^k / freq) < 2^32 (the error rcp * freq - 2^k is below freq <= 2^(k - 31), so
// x * error < 2^k).
__global__ __launch_bounds__(64) void spzw_normalise_kernel(const WStream* __restrict__ streams, const uint32_t* __restrict__ partial,
                                                            uint4* __restrict__ recs, uint8_t* __restrict__ tables, uint32_t* __restrict__ ns_out) {
    __shared__ uint32_t rem[256];
    __shared__ uint32_t present[256];
    const WStream st = streams[blockIdx.x];
    const int lane = threadIdx.x;
    if (st.count == 0) { if (lane == 0) ns_out[blockIdx.x] = 0; return; }
    uint32_t cnt[4] = {0, 0, 0, 0};
    for (uint32_t g = 0; g < st.nseg; ++g) {                       // segment order: fixed
        const uint4 v = reinterpret_cast<const uint4*>(partial + (size_t)(st.seg0 + g) * 256)[lane];
        cnt[0] += v.x; cnt[1] += v.y; cnt[2] += v.z; cnt[3] += v.w;
    }
    auto wave_sum = [](uint32_t v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        return v;
    };
    uint32_t mine = 0, top = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) if (cnt[r]) { ++mine; top = 4 * lane + r + 1; }
    const uint32_t nz = wave_sum(mine), spare = W_SCALE - nz, total = st.count;
    uint32_t f[4], fsum = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint64_t prod = (uint64_t)cnt[r] * spare;
        f[r] = cnt[r] ? 1u + (uint32_t)(prod / total) : 0u;
        rem[4 * lane + r] = (uint32_t)(prod % total);
        present[4 * lane + r] = cnt[r] ? 1u : 0u;
        fsum += f[r];
    }
    const uint32_t deficit = W_SCALE - wave_sum(fsum);             // < nz
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (!cnt[r]) continue;
        const uint32_t s = 4 * lane + r, my = rem[s];
        uint32_t rank = 0;
        for (uint32_t q = 0; q < 256; ++q) rank += (present[q] && (rem[q] > my || (rem[q] == my && q < s))) ? 1u : 0u;
        if (rank < deficit) ++f[r];
    }
    uint32_t lsum = f[0] + f[1] + f[2] + f[3], incl = lsum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    uint32_t cum = incl - lsum;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));
    const uint32_t ns = st.kind == JOB_PLANE ? 256u : top;         // the reference's tables end at the largest symbol seen
    uint8_t* tb = tables + (size_t)blockIdx.x * W_TABLE;
    if (lane == 0) { ns_out[blockIdx.x] = ns; tb[0] = (uint8_t)ns; tb[1] = (uint8_t)(ns >> 8); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t s = 4 * lane + r, fr = f[r];
        tb[2 + 2 * s] = (uint8_t)fr; tb[3 + 2 * s] = (uint8_t)(fr >> 8);
        uint4 rec = make_uint4(0, 0, 0, 0);
        if (fr) {
            const uint32_t sh = fr > 1 ? 32u - (uint32_t)__clz((int)(fr - 1)) : 0u, k = 31 + sh;
            rec = make_uint4(fr << 17, (uint32_t)((((uint64_t)1 << k) + fr - 1) / fr), fr | (k << 16), cum);
        }
        recs[(size_t)blockIdx.x * 256 + s] = rec;
        cum += fr;
    }
}

// One wavefront per stream, symbols taken last to first (rans.hpp:180-210, :269-279).  rANS is a serial recurrence on a 32-bit state:
// the state is UNIFORM across the wave, as in spz_rans_kernel -- every lane runs the same scalar program, the recurrence lives on
// the scalar ALU -- and the other lanes do the memory traffic around it, block by block from the end of the stream:
//   all lanes   read the block's W_B symbols from global memory, coalesced, and gather each symbol's encode record into LDS.  Unlike
//               the decoder, the encoder knows its symbols in advance: the table lookup is done here, in parallel, and is NOT on the
//               dependent chain
//   uniform     per symbol, from the block's last to its first: one LDS read of the staged record (its address does not depend on the
//               state), at most two renormalisation bytes (x < 2^31 and x_max >= 2^17), written BACKWARDS into an LDS block, then
//               x = (floor(x / f) << 14) + x mod f + cum with the division as a multiply and a shift
//   all lanes   flush the block's bytes, coalesced, below what the stream's scratch region already holds
// The region has 2 * count + 4 bytes and is filled from its end, so that the finished stream is its last `enc_size` bytes in file
// order: the four state bytes, most significant first (spz_rans_kernel reads them so), then the renormalisation bytes in decode
// order.  A block emits at most 2 * W_B (+ 4) bytes, a stream at most 2 * count + 4: neither buffer can overflow.
__global__ __launch_bounds__(64) void spzw_encode_kernel(const uint8_t* __restrict__ syms, const WStream* __restrict__ streams,
                                                         const uint4* __restrict__ recs, uint8_t* __restrict__ scratch,
                                                         uint32_t* __restrict__ enc_size) {
    __shared__ uint4 tab[256];
    __shared__ uint4 rbuf[W_B];
    __shared__ uint8_t obuf[W_OB + 4];
    const WStream st = streams[blockIdx.x];
    const int lane = threadIdx.x;
    if (st.count == 0) { if (lane == 0) enc_size[blockIdx.x] = 0; return; }
#pragma unroll
    for (int r = 0; r < 4; ++r) tab[lane + 64 * r] = recs[(size_t)blockIdx.x * 256 + lane + 64 * r];
    const uint8_t* p = syms + st.sym_off;
    uint8_t* region = scratch + st.scratch_off;
    const uint64_t cap = 2ull * st.count + 4;
    uint64_t gpos = cap;                                            // the region is full from here on
    uint32_t x = W_L;
    for (int64_t base = (int64_t)((st.count - 1) / W_B) * W_B; base >= 0; base -= W_B) {
        const int cnt = (int)min((int64_t)W_B, (int64_t)st.count - base);
        __syncthreads();                                            // tab is written; the previous flush has read obuf
        for (int i = lane; i < cnt; i += 64) rbuf[i] = tab[p[base + i]];
        __syncthreads();
        int opos = W_OB;
        for (int i = cnt - 1; i >= 0; --i) {
            const uint4 r = rbuf[i];
            const uint32_t xmax = w_rfl(r.x), rcp = w_rfl(r.y), fk = w_rfl(r.z), cum = w_rfl(r.w);
            if (x >= xmax) {
                obuf[--opos] = (uint8_t)x; x >>= 8;                 // all lanes, same value, same address
                if (x >= xmax) { obuf[--opos] = (uint8_t)x; x >>= 8; }
            }
            const uint32_t q = (uint32_t)(((uint64_t)x * rcp) >> (fk >> 16));
            x = (q << W_PROB_BITS) + (x - q * (fk & 0xFFFFu)) + cum;
        }
        if (base == 0) {                                            // rans.hpp:198-203: low byte first, then the whole output is reversed
#pragma unroll
            for (int b = 0; b < 4; ++b) { obuf[--opos] = (uint8_t)x; x >>= 8; }
        }
        __syncthreads();
        const int len = W_OB - opos;
        gpos -= (uint64_t)len;
        for (int i = lane; i < len; i += 64) region[gpos + i] = obuf[opos + i];
    }
    if (lane == 0) enc_size[blockIdx.x] = (uint32_t)(cap - gpos);
}

// Varint escapes of a gap or integer stream (sparsepress_v2.hpp:116-120, :191-195), in forward order, which is the order the decoders
// consume them in.  One workgroup per stream walks it 256 elements at a time: every lane takes the length of its element's varint (0
// when it is no escape), wave and workgroup prefix sums place it, the running total carries to the next tile.  The bytes written are
// exactly what spzw_symbolise_kernel counted with the same length rule, which is what the stream's escape region was sized by.
__global__ __launch_bounds__(256) void spzw_escape_kernel(const uint32_t* __restrict__ gaps, const uint32_t* __restrict__ ivals,
                                                          const WStream* __restrict__ streams, const unsigned long long* __restrict__ esc_bytes,
                                                          uint8_t* __restrict__ esc) {
    __shared__ uint32_t wsum[4];
    const WStream st = streams[blockIdx.x];
    if (st.kind == JOB_PLANE || st.count == 0 || esc_bytes[blockIdx.x] == 0) return;
    const uint32_t* src = (st.kind == JOB_GAPS ? gaps : ivals) + st.src_off;
    uint8_t* out = esc + st.esc_off;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint64_t carry = 0;
    for (uint32_t t0 = 0; t0 < st.count; t0 += 256) {
        const uint32_t t = t0 + tid;
        uint32_t v = t < st.count ? src[t] : 0u;
        const uint32_t len = v >= 255u ? w_varint_len(v) : 0u;
        uint32_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; tile += wsum[w]; }
        uint8_t* o = out + carry + before + (incl - len);
        for (uint32_t b = 0; b + 1 < len; ++b) { *o++ = (uint8_t)(v | 0x80u); v >>= 7; }
        if (len) *o = (uint8_t)v;
        carry += tile;
        __syncthreads();                                            // wsum is rewritten by the next tile
    }
}

// One workgroup per piece of at most W_PIECE bytes: tables, rANS bytes and escapes into the data section
__global__ __launch_bounds__(256) void spzw_gather_kernel(const WCopy* __restrict__ copies, const uint8_t* __restrict__ tables,
                                                          const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ esc,
                                                          uint8_t* __restrict__ data) {
    const WCopy c = copies[blockIdx.x];
    const uint8_t* src = (c.which == 0 ? tables : c.which == 1 ? scratch : esc) + c.src;
    uint8_t* dst = data + c.dst;
    for (uint32_t i = threadIdx.x; i < c.len; i += 256) dst[i] = src[i];
}

}  // namespace rcppml_spzw
