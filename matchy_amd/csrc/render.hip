// Rendered records, on the GPU: the final records of a fetch as NDJSON, one line per record in the order of the arrays the caller
// gets, written into one block in device memory. What a byte of the text is decides render_core.h; this file decides who computes it.
//   k_rd_classify       one lane per record. From sizes that are known without reading the batch it decides SHORT or LONG. A short
//                       record is measured here, by its lane; a long one goes onto the long list and reserves its piece slots
//   k_rd_piece_measure  one wave per piece of a long record's "input_line" / "matched_text": the length of the piece's text
//   k_rd_long_measure   one wave per long record: walks the parts of the record, the lanes sharing payload lookups; where a cut field
//                       stands it turns the lengths of its pieces into their offsets inside the record
//   k_rd_chunk_sum      } exclusive prefix of the record lengths in 64 bits (the shape of k_line_chunk_sum / k_line_scan): rec_off,
//   k_rd_scan           } and the demand of the block
//   k_rd_write_short    short records: a wave stages the text of its 64 records in LDS, window by window, and stores it with aligned
//                       16-byte stores
//   k_rd_write_long     long records: one wave writes everything but the cut fields, one wave per piece writes the piece
// Every store to the block sits behind min(demand, capacity); the long list behind the record count, the piece arrays behind
// piece_cap, the miss list behind miss_cap. Hits and lines are clamped to the batch before they are read: no load reaches data + len.
// Every loop names its bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "render.h"
#include "render_core.h"

namespace mxy {

namespace {

namespace R = render;

constexpr uint32_t RD_THREADS = 256, RD_WAVES = RD_THREADS / 64;
constexpr uint32_t RD_ITEMS = RENDER_SCAN_CHUNK / RD_THREADS;
constexpr uint32_t RD_GRID_X = 256, RD_GRID_Y = 32;   // long records side by side, and workgroups that share the pieces of one
constexpr uint32_t RD_STAGE = 8192;                  // bytes of the block a wave stages in LDS per turn (k_rd_write_short)
static_assert(RD_STAGE % 1024 == 0, "whole 16-byte stores of 64 lanes");
constexpr uint32_t RD_MISS_PROBES = 64;               // slots of the miss set a lane looks at before it appends without a claim
constexpr uint64_t RD_LONG_BIT = 1ull << 63;          // in rec_len: the record is on the long list (not part of its length)
static_assert(RENDER_SCAN_CHUNK % RD_THREADS == 0, "whole entries per thread");
static_assert(RENDER_PIECE % 64 == 0, "whole steps of a wave per piece");

// ------------------------------------------------------------------------------------------------ records
struct Rec { uint32_t start, len, value, n_ids, kind, prefix; };

__device__ __forceinline__ Rec load_rec(const RenderInput& in, uint32_t i) {
    Rec r;
    if (i < in.b.n_fin) {
        const uint4 v = reinterpret_cast<const uint4*>(in.b.fin)[i];
        r.start = v.x; r.len = v.y & 0xFFFFFFu; r.value = v.z; r.kind = v.w & 0xFFu; r.prefix = (v.w >> 8) & 0xFFu; r.n_ids = v.w >> 16;
    } else {   // compact IPv4 (matchy_scan_ip4_hit_expand)
        const uint2 c = reinterpret_cast<const uint2*>(in.b.c4)[i - in.b.n_fin];
        r.start = c.x; r.len = ((c.y >> 22) & 15u) + 7u; r.value = c.y & ((1u << 22) - 1u); r.kind = 2; r.prefix = c.y >> 26; r.n_ids = 0;
    }
    if (r.kind == 2) r.n_ids = 0;
    // inside the batch, whatever the record says
    r.start = min(r.start, in.b.len);
    r.len = min(r.len, in.b.len - r.start);
    return r;
}

__device__ __forceinline__ R::RecordIn record_in(const RenderInput& in, uint32_t i, const Rec& rc) {
    R::RecordIn r;
    r.hit = in.b.data + rc.start; r.hit_len = rc.len;
    r.value = rc.value; r.n_ids = rc.n_ids; r.kind = (uint8_t)rc.kind; r.prefix_len = (uint8_t)rc.prefix;
    r.flags = in.flags;
    uint32_t seg = 0;
    if (in.n_segments) {
        seg = i < in.b.n_fin ? in.seg_of_fin[i] : in.seg_of_c4[i - in.b.n_fin];
        if (seg >= in.n_segments) seg = in.n_segments - 1u;
    }
    r.line = in.b.data; r.line_len = 0; r.line_number = 0;
    if (in.flags & (R::FLAG_LINE_NUMBERS | R::FLAG_INPUT_LINE)) {
        const uint4 v = *reinterpret_cast<const uint4*>(i < in.b.n_fin ? in.fin_lines + i : in.c4_lines + (i - in.b.n_fin));
        const uint32_t ls = min(v.y, in.b.len), le = min(max(v.z, ls), in.b.len);
        r.line = in.b.data + ls; r.line_len = le - ls;
        const uint32_t first = in.n_segments && in.seg_line_base ? in.seg_line_base[seg] : 0u;
        r.line_number = in.line_bases[seg] + (uint64_t)(v.x - first) + 1u;
    }
    const RenderSource s = in.sources[seg];
    r.source = in.source_text + s.off; r.source_len = s.len;
    return r;
}

// the source bytes of a record that a lane would have to walk, from sizes alone
__device__ __forceinline__ bool is_short(const RenderInput& in, const R::RecordIn& r) {
    const uint64_t bytes = (uint64_t)r.hit_len + ((in.flags & R::FLAG_INPUT_LINE) ? r.line_len : 0u);
    return bytes <= RENDER_SHORT_MAX && r.n_ids <= RENDER_SHORT_IDS;
}

// ------------------------------------------------------------------------------------------------ payload table, miss list
__device__ __forceinline__ bool table_find(const PayloadTable& t, uint32_t key, uint32_t& off, uint32_t& len) {
    if (!t.n_slots) return false;
    uint32_t s = payload_slot(key, t.n_slots);
    for (uint32_t p = 0; p < t.n_slots; ++p) {   // bound: the slots of the table (it is at most half full: an empty slot ends the walk)
        const uint4 v = *reinterpret_cast<const uint4*>(t.slots + s);
        if (v.x == key) { off = v.y; len = v.z; return true; }
        if (v.x == RENDER_KEY_EMPTY) return false;
        s = (s + 1u) & (t.n_slots - 1u);
    }
    return false;
}

// The list holds a data offset once: the lane that claims the offset's slot in the per-scan set appends it. A lane that finds no
// slot within RD_MISS_PROBES appends without a claim (the host renders an offset once however often it is listed).
__device__ __forceinline__ void miss_add(const RenderWork& w, uint32_t key) {
    bool fresh = true;
    if (w.miss_set_slots) {
        uint32_t s = payload_slot(key, w.miss_set_slots);
        for (uint32_t p = 0; p < RD_MISS_PROBES && p < w.miss_set_slots; ++p) {   // bound: RD_MISS_PROBES
            const uint32_t cur = atomicCAS(&w.miss_set[s], RENDER_KEY_EMPTY, key);
            if (cur == RENDER_KEY_EMPTY) break;
            if (cur == key) { fresh = false; break; }
            s = (s + 1u) & (w.miss_set_slots - 1u);
        }
    }
    if (!fresh) return;
    const uint32_t at = atomicAdd(&w.miss->misses, 1u);   // counts past the capacity
    if (at < w.miss_cap) w.miss_list[at] = key;
}

// payloads as one lane sees them (short records: at most RENDER_SHORT_IDS ids). measure: misses go onto the list.
struct LanePayloads {
    const RenderInput& in;
    const PayloadTable& t;
    const RenderWork* w;   // null while writing
    template <class S>
    __device__ void one(S& s, uint32_t key) {
        uint32_t off, len;
        if (table_find(t, key, off, len)) s.bytes(t.pool + off, len);
        else if (w) miss_add(*w, key);
    }
    template <class S>
    __device__ void array(S& s, uint32_t first, uint32_t n) {
        bool any = false;
        for (uint32_t k = 0; k < n && k < RENDER_SHORT_IDS; ++k) {   // bound: RENDER_SHORT_IDS
            if ((uint64_t)first + k >= in.n_data_offsets) break;
            const int64_t d = in.data_offsets[first + k];
            if (d < 0) continue;
            if (any) MXY_RC_LIT(s, ","); else MXY_RC_LIT(s, "\"data\":[");
            one(s, (uint32_t)d);
            any = true;
        }
        if (any) MXY_RC_LIT(s, "],");
    }
};

// ------------------------------------------------------------------------------------------------ a wave at work
__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t wave_incl(uint64_t v) {
    const uint32_t lane = lane_id();
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, off);
        if (lane >= off) v += t;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_last(uint64_t incl) { return (uint64_t)__shfl((unsigned long long)incl, 63); }

// one entry of a payload array as the wave sees it: lane k of a step holds id first + base + k
struct IdText { bool valid; uint32_t off, len; };
__device__ __forceinline__ IdText id_text(const RenderInput& in, const PayloadTable& t, const RenderWork* w, uint32_t first, uint32_t k, uint32_t n) {
    IdText e{false, 0, 0};
    if (k >= n || (uint64_t)first + k >= in.n_data_offsets) return e;
    const int64_t d = in.data_offsets[first + k];
    if (d < 0) return e;
    e.valid = true;
    if (!table_find(t, (uint32_t)d, e.off, e.len)) { e.off = 0; e.len = 0; if (w) miss_add(*w, (uint32_t)d); }
    return e;
}

// Measures a long record: every lane of the wave calls the same members with the same arguments. Where a cut field stands, the
// lengths of its pieces (k_rd_piece_measure) become offsets from the beginning of the record.
struct WaveLenSink {
    uint64_t n;
    const uint32_t* piece_len;
    uint64_t* piece_off;
    uint32_t pb, np_line, np_hit;
    __device__ void lit(const char*, uint32_t len) { n += len; }
    __device__ void bytes(const uint8_t*, uint32_t len) { n += len; }
    __device__ void dec(uint64_t v) { n += R::dec_len(v); }
    __device__ void text_inline(const uint8_t* f, uint32_t len) {
        uint64_t t = 0;
        for (uint32_t i = lane_id(); i < len; i += 64u) t += R::esc_len(f[i]);   // bound: the 24-bit length of a hit, 64 bytes a step
        n += wave_last(wave_incl(t));
    }
    __device__ void pieces(uint32_t first, uint32_t np) {
        for (uint32_t base = 0; base < np; base += 64u) {   // bound: the pieces of a field, at most 2^31 / RENDER_PIECE, 64 a step
            const uint32_t p = base + lane_id();
            const uint64_t v = p < np ? piece_len[first + p] : 0u;
            const uint64_t incl = wave_incl(v);
            if (p < np) piece_off[first + p] = n + incl - v;
            n += wave_last(incl);
        }
    }
    __device__ void line(const uint8_t*, uint32_t) { pieces(pb, np_line); }
    __device__ void text(const uint8_t*, uint32_t) { pieces(pb + np_line, np_hit); }
};

// `len` bytes from `src` (any alignment; the pool, the source text) to o[at ..) by the 64 lanes of a wave, o 16-byte aligned: the
// bytes up to the block's next 16-byte boundary and the ragged end one byte per lane, the body as 16-byte stores at aligned addresses
// of the block, each fed by one 16-byte load that lies wholly inside [src, src + len). No store at or behind `end`.
__device__ __forceinline__ void wave_copy(uint8_t* __restrict__ o, uint64_t end, uint64_t at, const uint8_t* __restrict__ src, uint32_t len) {
    const uint32_t lane = lane_id();
    const uint32_t head = min(len, (uint32_t)((16u - (uint32_t)(at & 15u)) & 15u));   // at most 15 bytes
    if (lane < head && at + lane < end) o[at + lane] = src[lane];
    const uint32_t units = (len - head) / 16u;
    for (uint32_t u = lane; u < units; u += 64u) {   // bound: len / 1024 steps
        const uint64_t d = at + head + 16ull * u;
        const uint8_t* s = src + head + 16u * u;
        if (d + 16u <= end) {
            uint4 v;
            __builtin_memcpy(&v, s, 16);
            *reinterpret_cast<uint4*>(o + d) = v;
        } else for (uint32_t k = 0; k < 16u; ++k) if (d + k < end) o[d + k] = s[k];   // the unit the end cuts
    }
    const uint32_t done = head + 16u * units;   // at most 15 bytes are left
    if (done + lane < len && at + done + lane < end) o[at + done + lane] = src[done + lane];
}

// Writes a long record but for its cut fields, whose pieces other waves write: their room is skipped.
struct WavePutSink {
    uint8_t* o;
    uint64_t pos, end;
    uint64_t after_line, after_hit;   // where the record goes on behind each cut field
    bool cut_line, cut_hit;           // the field has pieces (an empty field has none: the record goes on where it stands)
    __device__ void put(const uint8_t* p, uint32_t len) {
        for (uint32_t k = lane_id(); k < len; k += 64u) if (pos + k < end) o[pos + k] = p[k];   // bound: len, 64 bytes a step
        pos += len;
    }
    __device__ void lit(const char* p, uint32_t len) { put(reinterpret_cast<const uint8_t*>(p), len); }
    __device__ void bytes(const uint8_t* p, uint32_t len) { wave_copy(o, end, pos, p, len); pos += len; }   // payload JSON, the source
    __device__ void dec(uint64_t v) { uint8_t t[20]; put(t, R::dec_put(v, t)); }
    __device__ void text_inline(const uint8_t* f, uint32_t len) {
        uint8_t t[R::BYTE_TEXT_MAX];
        for (uint32_t base = 0; base < len; base += 64u) {   // bound: the 24-bit length of a hit, 64 bytes a step
            const uint32_t i = base + lane_id();
            const uint32_t k = i < len ? R::esc_put(f[i], t) : 0u;
            const uint64_t incl = wave_incl(k);
            for (uint32_t j = 0; j < k; ++j) if (pos + incl - k + j < end) o[pos + incl - k + j] = t[j];   // bound: BYTE_TEXT_MAX
            pos += wave_last(incl);
        }
    }
    __device__ void line(const uint8_t*, uint32_t) { if (cut_line) pos = after_line; }
    __device__ void text(const uint8_t*, uint32_t) { if (cut_hit) pos = after_hit; }
};

// payloads as a wave sees them: the lanes look the ids up side by side
struct WavePayloads {
    const RenderInput& in;
    const PayloadTable& t;
    const RenderWork* w;      // null while writing
    uint32_t* status;         // measure: RENDER_TOO_LARGE for an array beyond RENDER_PAYLOAD_ARRAY_MAX
    template <class S>
    __device__ void one(S& s, uint32_t key) {
        uint32_t off = 0, len = 0;
        const bool found = table_find(t, key, off, len);
        if (found) s.bytes(t.pool + off, len);
        else if (w && lane_id() == 0) miss_add(*w, key);
    }
    // `"data":` then one byte ('[' in front of the first, ',' in front of every other) and the text per id with data, then `],`
    __device__ void array(WaveLenSink& s, uint32_t first, uint32_t n) {
        uint64_t total = 0;
        for (uint32_t base = 0; base < n; base += 64u) {   // bound: the 16-bit id count, 64 ids a step
            const IdText e = id_text(in, t, w, first, base + lane_id(), n);
            total += wave_last(wave_incl(e.valid ? 1ull + e.len : 0ull));
        }
        if (total > RENDER_PAYLOAD_ARRAY_MAX && lane_id() == 0) atomicMax(status, RENDER_TOO_LARGE);
        if (total) s.n += 7u + total + 2u;
    }
    __device__ void array(WavePutSink& s, uint32_t first, uint32_t n) {
        bool any = false;
        for (uint32_t base = 0; base < n; base += 64u) {   // bound: the 16-bit id count, 64 ids a step
            const IdText e = id_text(in, t, nullptr, first, base + lane_id(), n);
            const uint64_t mine = e.valid ? 1ull + e.len : 0ull, incl = wave_incl(mine), step = wave_last(incl);
            if (!step) continue;
            if (!any) MXY_RC_LIT(s, "\"data\":");
            const unsigned long long have = __ballot(e.valid);
            const uint32_t lead = (uint32_t)__ffsll((long long)have) - 1u;   // the first id with data of this step
            const uint64_t at = s.pos + incl - mine;
            if (e.valid && at < s.end) s.o[at] = (!any && lane_id() == lead) ? '[' : ',';
            for (uint32_t k = 0; k < 64u; ++k) {   // bound: the lanes of a wave; the text of each id by all lanes, 64 bytes a step
                const uint32_t len_k = __shfl(e.valid ? e.len : 0u, k);
                if (!len_k) continue;
                const uint32_t off_k = __shfl(e.off, k);
                const uint64_t at_k = (uint64_t)__shfl((unsigned long long)at, k) + 1u;
                wave_copy(s.o, s.end, at_k, t.pool + off_k, len_k);
            }
            s.pos += step;
            any = true;
        }
        if (any) MXY_RC_LIT(s, "],");
    }
};

// ------------------------------------------------------------------------------------------------ measure
__global__ __launch_bounds__(RD_THREADS) void k_rd_classify(RenderInput in, PayloadTable t, RenderWork w, uint32_t n) {
    const uint32_t i = blockIdx.x * RD_THREADS + threadIdx.x;
    bool counted = false;
    if (i < n) {
        const Rec rc = load_rec(in, i);
        const R::RecordIn r = record_in(in, i, rc);
        if (is_short(in, r)) {
            R::LenSink s;
            LanePayloads pay{in, t, &w};
            // bound: RENDER_SHORT_MAX source bytes, RENDER_SHORT_IDS lookups; payload bytes are counted here, not walked
            R::record_emit(r, pay, s);
            if (s.n <= RENDER_SHORT_TEXT) {   // what its lane will write: bounded, whatever the payloads are
                w.rec_len[i] = s.n;
                counted = true;
            }
        }
        if (!counted) {
            const uint32_t np_line = (in.flags & R::FLAG_INPUT_LINE) ? render_pieces(r.line_len) : 0u, np_hit = render_pieces(r.hit_len);
            const uint32_t at = atomicAdd(&w.ctr->n_long, 1u);             // never more than n
            // counts past piece_cap, in 64 bits: every hit of a long line asks for the line's pieces again
            const uint64_t pb = atomicAdd(reinterpret_cast<unsigned long long*>(&w.ctr->n_pieces), (unsigned long long)(np_line + np_hit));
            const bool fits = pb + np_line + np_hit <= w.piece_cap;
            if (!fits) atomicMax(&w.ctr->pieces_short, 1u);
            if (at < n) w.long_list[at] = RenderLong{i, fits ? (uint32_t)pb : 0xFFFFFFFFu, np_line, np_hit};
            w.rec_len[i] = RD_LONG_BIT;   // its length follows in k_rd_long_measure
        }
    }
    const unsigned long long shorts = __ballot(counted);
    if (lane_id() == 0 && shorts) atomicAdd(&w.ctr->n_short, (uint32_t)__popcll(shorts));
}

// the field and the byte range of piece u (0 .. np_line + np_hit - 1) of a long record
struct Piece { const uint8_t* f; uint32_t n, a, b; bool is_line; };
__device__ __forceinline__ Piece piece_of(const R::RecordIn& r, const RenderLong& l, uint32_t u) {
    Piece p;
    p.is_line = u < l.np_line;
    p.f = p.is_line ? r.line : r.hit;
    p.n = p.is_line ? r.line_len : r.hit_len;
    const uint32_t k = p.is_line ? u : u - l.np_line;
    p.a = k * RENDER_PIECE;   // k < n / RENDER_PIECE + 1: no overflow
    p.b = min(p.n, p.a + RENDER_PIECE);
    return p;
}
__device__ __forceinline__ bool pieces_fit(const RenderLong& l, uint32_t piece_cap) { return l.piece_base != 0xFFFFFFFFu && (uint64_t)l.piece_base + l.np_line + l.np_hit <= piece_cap; }

__global__ __launch_bounds__(RD_THREADS) void k_rd_piece_measure(RenderInput in, RenderWork w, uint32_t n) {
    const uint32_t n_long = min(w.ctr->n_long, n);
    for (uint32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // bound: the long list
        const RenderLong l = w.long_list[li];
        if (!pieces_fit(l, w.piece_cap)) continue;
        const R::RecordIn r = record_in(in, l.rec, load_rec(in, l.rec));
        for (uint32_t u = blockIdx.y * RD_WAVES + (threadIdx.x >> 6); u < l.np_line + l.np_hit; u += gridDim.y * RD_WAVES) {   // bound: the record's pieces
            const Piece p = piece_of(r, l, u);
            uint32_t t = 0;
            for (uint32_t i = p.a + lane_id(); i < p.b; i += 64u)   // bound: RENDER_PIECE / 64 steps
                t += p.is_line ? R::line_byte_len(p.f, p.n, i) : R::esc_len(p.f[i]);
            const uint64_t sum = wave_last(wave_incl(t));
            if (lane_id() == 0) w.piece_len[l.piece_base + u] = (uint32_t)sum;   // at most BYTE_TEXT_MAX * RENDER_PIECE
        }
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_rd_long_measure(RenderInput in, PayloadTable t, RenderWork w, uint32_t n) {
    const uint32_t n_long = min(w.ctr->n_long, n);
    const uint32_t wave = blockIdx.x * RD_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * RD_WAVES;
    for (uint32_t li = wave; li < n_long; li += n_waves) {   // bound: the long list
        const RenderLong l = w.long_list[li];
        if (!pieces_fit(l, w.piece_cap)) continue;   // rec_len stays 0: nothing of it is written, and the host repeats the measure
        const R::RecordIn r = record_in(in, l.rec, load_rec(in, l.rec));
        WaveLenSink s{0, w.piece_len, w.piece_off, l.piece_base, l.np_line, l.np_hit};
        WavePayloads pay{in, t, &w, &w.ctr->status};
        R::record_emit(r, pay, s);
        if (lane_id() == 0) w.rec_len[l.rec] = s.n | RD_LONG_BIT;
    }
}

// ------------------------------------------------------------------------------------------------ offsets
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* s) {
    v = wave_last(wave_incl(v));
    if (lane_id() == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < RD_WAVES; ++k) t += s[k];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(RD_THREADS) void k_rd_chunk_sum(const uint64_t* __restrict__ rec_len, uint32_t n, uint64_t* __restrict__ chunk_sums) {
    __shared__ uint64_t s[RD_WAVES];
    const uint32_t first = blockIdx.x * RENDER_SCAN_CHUNK;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < RD_ITEMS; ++r) {
        const uint32_t i = first + r * RD_THREADS + threadIdx.x;
        if (i < n) v += rec_len[i] & ~RD_LONG_BIT;
    }
    v = block_sum(v, s);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = v;
}

// rec_off[i] = sum of the lengths in front of record i, i = 0 .. n; the total is the demand
__global__ __launch_bounds__(RD_THREADS) void k_rd_scan(const uint64_t* __restrict__ rec_len, uint32_t n, const uint64_t* __restrict__ chunk_sums,
                                                        uint64_t* __restrict__ rec_off, RenderCounters* __restrict__ ctr, uint64_t max_bytes) {
    __shared__ uint64_t s[RD_THREADS];
    __shared__ uint64_t sw[RD_WAVES];
    if (n == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { rec_off[0] = 0; ctr->demand = 0; }
        return;
    }
    uint64_t before = 0;
    for (uint32_t c = threadIdx.x; c < blockIdx.x; c += RD_THREADS) before += chunk_sums[c];   // bound: the chunks in front
    before = block_sum(before, sw);
    const uint32_t i0 = blockIdx.x * RENDER_SCAN_CHUNK + threadIdx.x * RD_ITEMS;
    uint64_t c[RD_ITEMS], own = 0;
#pragma unroll
    for (uint32_t r = 0; r < RD_ITEMS; ++r) { c[r] = i0 + r < n ? rec_len[i0 + r] & ~RD_LONG_BIT : 0ull; own += c[r]; }
    s[threadIdx.x] = own;
    __syncthreads();
    uint64_t incl = own;
    for (uint32_t off = 1; off < RD_THREADS; off <<= 1) {
        const uint64_t v = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        incl += v;
        s[threadIdx.x] = incl;
        __syncthreads();
    }
    uint64_t run = before + incl - own;
#pragma unroll
    for (uint32_t r = 0; r < RD_ITEMS; ++r) {
        if (i0 + r < n) rec_off[i0 + r] = run;
        run += c[r];
        if (i0 + r + 1 == n) {
            rec_off[n] = run;
            ctr->demand = run;
            if (run > max_bytes) atomicMax(&ctr->status, RENDER_TOO_LARGE);
        }
    }
}

// ------------------------------------------------------------------------------------------------ write
// A lane's record into the window [w0, w0 + RD_STAGE) of the block that its wave stages in LDS; bytes outside the window are dropped.
struct StageSink {
    uint8_t* lds;
    uint64_t pos, w0;
    __device__ void put(const uint8_t* p, uint32_t len) {
        if (pos + len > w0 && pos < w0 + RD_STAGE)
            for (uint32_t k = 0; k < len; ++k) { const uint64_t q = pos + k - w0; if (pos + k >= w0 && q < RD_STAGE) lds[q] = p[k]; }   // bound: len
        pos += len;
    }
    __device__ void lit(const char* p, uint32_t len) { put(reinterpret_cast<const uint8_t*>(p), len); }
    __device__ void bytes(const uint8_t* p, uint32_t len) { put(p, len); }
    __device__ void text(const uint8_t* f, uint32_t len) {
        uint8_t t[R::BYTE_TEXT_MAX];
        for (uint32_t i = 0; i < len; ++i) put(t, R::esc_put(f[i], t));   // bound: RENDER_SHORT_MAX
    }
    __device__ void text_inline(const uint8_t* f, uint32_t len) { text(f, len); }
    __device__ void line(const uint8_t* f, uint32_t len) {
        uint8_t t[R::BYTE_TEXT_MAX];
        for (uint32_t i = 0; i < len; ++i) put(t, R::line_byte_put(f, len, i, t));   // bound: RENDER_SHORT_MAX
    }
    __device__ void dec(uint64_t v) { uint8_t t[20]; put(t, R::dec_put(v, t)); }
};

// the lanes of a wave have written LDS that other lanes of the same wave read next (and the other way round)
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Short records. The records of a wave's 64 lanes lie side by side in the block (a long record among them is a hole that
// k_rd_write_long fills), so the wave takes each run of consecutive short records as one range of the block: window by window of
// RD_STAGE bytes, every lane of the run puts what its record has inside the window into LDS, then the wave stores the window —
// the bytes up to the block's next 16-byte boundary and the ragged end one byte per lane, the body as 16-byte stores, contiguous
// over the lanes. No store at or behind min(demand, capacity).
__global__ __launch_bounds__(RD_THREADS) void k_rd_write_short(RenderInput in, PayloadTable t, RenderWork w, uint32_t n, uint8_t* __restrict__ text, uint64_t capacity) {
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[RD_WAVES][RD_STAGE];
    if (w.ctr->status != RENDER_OK || w.ctr->pieces_short) return;
    uint8_t* stage = stage_all[threadIdx.x >> 6];
    const uint32_t i = blockIdx.x * RD_THREADS + threadIdx.x, lane = lane_id();
    const uint64_t end = min64(w.ctr->demand, capacity);   // no store at or behind it
    uint64_t lo = 0, hi = 0;
    bool mine = false;
    if (i < n) {
        const uint64_t len = w.rec_len[i];
        mine = !(len & RD_LONG_BIT);
        if (mine) { lo = w.rec_off[i]; hi = lo + len; }
    }
    unsigned long long left = __ballot(mine);
    while (left) {   // bound: the runs of short records among 64 lanes, at most 32
        const uint32_t a = (uint32_t)__ffsll((long long)left) - 1u;
        const unsigned long long gap = ~(left >> a);   // bit k: lane a + k is not short
        const uint32_t b = gap ? a + (uint32_t)__ffsll((long long)gap) - 1u : 64u;   // the run is lanes a .. b - 1
        left &= b >= 64u ? 0ull : ~0ull << b;
        const uint64_t run_lo = (uint64_t)__shfl((unsigned long long)lo, (int)a);
        const uint64_t run_hi = min64((uint64_t)__shfl((unsigned long long)hi, (int)(b - 1u)), end);
        const bool in_run = lane >= a && lane < b;
        if (run_lo >= run_hi) continue;   // the run begins at or behind the end (a block that is too small): nothing of it is stored
        for (uint64_t w0 = run_lo & ~15ull; w0 < run_hi; w0 += RD_STAGE) {   // bound: the text of at most 64 short records / RD_STAGE
            if (in_run && hi > w0 && lo < w0 + RD_STAGE) {
                const R::RecordIn r = record_in(in, i, load_rec(in, i));
                StageSink s{stage, lo, w0};
                LanePayloads pay{in, t, nullptr};
                R::record_emit(r, pay, s);   // bound: RENDER_SHORT_TEXT bytes of text (k_rd_classify sent longer records to the long list)
            }
            wave_sync_lds();
            const uint64_t f_lo = run_lo > w0 ? run_lo : w0, f_hi = min64(run_hi, w0 + RD_STAGE);
            const uint64_t head_end = min64(f_hi, (f_lo + 15ull) & ~15ull);   // at most 15 bytes
            if (f_lo + lane < head_end) text[f_lo + lane] = stage[f_lo + lane - w0];   // f_lo < f_hi in every window: w0 < run_hi and run_lo < run_hi
            const uint64_t body_end = f_hi & ~15ull;
            for (uint64_t p = head_end + lane * 16ull; p + 16ull <= body_end; p += 64ull * 16ull)   // bound: RD_STAGE / 1024 steps
                *reinterpret_cast<uint4*>(text + p) = *reinterpret_cast<const uint4*>(stage + (p - w0));
            const uint64_t tail = body_end > head_end ? body_end : head_end;   // at most 15 bytes
            if (tail + lane < f_hi) text[tail + lane] = stage[tail + lane - w0];
            wave_sync_lds();
        }
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_rd_write_long(RenderInput in, PayloadTable t, RenderWork w, uint32_t n, uint8_t* __restrict__ text, uint64_t capacity) {
    if (w.ctr->status != RENDER_OK || w.ctr->pieces_short) return;
    const uint32_t n_long = min(w.ctr->n_long, n);
    const uint64_t end = min64(w.ctr->demand, capacity);   // no store at or behind it
    for (uint32_t li = blockIdx.x; li < n_long; li += gridDim.x) {   // bound: the long list
        const RenderLong l = w.long_list[li];
        const uint64_t rec_at = w.rec_off[l.rec];
        if (rec_at >= end) continue;
        const R::RecordIn r = record_in(in, l.rec, load_rec(in, l.rec));
        const uint32_t np = l.np_line + l.np_hit;
        // unit 0: the record but for its cut fields; unit 1 + u: piece u
        for (uint32_t unit = blockIdx.y * RD_WAVES + (threadIdx.x >> 6); unit < np + 1u; unit += gridDim.y * RD_WAVES) {   // bound: the record's pieces + 1
            if (unit == 0) {
                // behind a cut field the record goes on where its last piece ends
                uint64_t after_line = 0, after_hit = 0;
                if (l.np_line) after_line = rec_at + w.piece_off[l.piece_base + l.np_line - 1u] + w.piece_len[l.piece_base + l.np_line - 1u];
                if (l.np_hit) after_hit = rec_at + w.piece_off[l.piece_base + np - 1u] + w.piece_len[l.piece_base + np - 1u];
                WavePutSink s{text, rec_at, end, after_line, after_hit, l.np_line != 0, l.np_hit != 0};
                WavePayloads pay{in, t, nullptr, nullptr};
                R::record_emit(r, pay, s);
                continue;
            }
            const uint32_t u = unit - 1u;
            const Piece p = piece_of(r, l, u);
            uint64_t pos = rec_at + w.piece_off[l.piece_base + u];
            uint8_t tb[R::BYTE_TEXT_MAX];
            for (uint32_t base = p.a; base < p.b; base += 64u) {   // bound: RENDER_PIECE / 64 steps
                const uint32_t i = base + lane_id();
                const uint32_t k = i >= p.b ? 0u : p.is_line ? R::line_byte_put(p.f, p.n, i, tb) : R::esc_put(p.f[i], tb);
                const uint64_t incl = wave_incl(k);
                for (uint32_t j = 0; j < k; ++j) if (pos + incl - k + j < end) text[pos + incl - k + j] = tb[j];   // bound: BYTE_TEXT_MAX
                pos += wave_last(incl);
            }
        }
    }
}

}  // namespace

uint32_t render_chunks(uint32_t n) { return std::max<uint32_t>(1u, (uint32_t)(((uint64_t)n + RENDER_SCAN_CHUNK - 1) / RENDER_SCAN_CHUNK)); }

static dim3 long_grid(uint32_t n, uint32_t long_hint) {
    // the records of the long list side by side whatever the scan before had; the hint only says whether a record's pieces are worth
    // more than one workgroup
    return dim3(std::min(n, RD_GRID_X), long_hint ? RD_GRID_Y : 1u);
}

static uint32_t record_count(const RenderInput& in, bool& ok) {
    ok = (uint64_t)in.b.n_fin + in.b.n_c4 <= 0xFFFFFFFFull;
    return in.b.n_fin + in.b.n_c4;
}

hipError_t render_measure(const RenderInput& in, const PayloadTable& table, const RenderWork& w, uint64_t max_bytes, int n_cu, hipStream_t stream) {
    bool ok;
    const uint32_t n = record_count(in, ok);
    if (!ok || (table.n_slots & (table.n_slots - 1u)) || (w.miss_set_slots & (w.miss_set_slots - 1u))) return hipErrorInvalidValue;
    if (n) {
        hipLaunchKernelGGL(k_rd_classify, dim3((n + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, stream, in, table, w, n);
        // few records are long: the workgroups leave at once where the list is empty
        hipLaunchKernelGGL(k_rd_piece_measure, long_grid(n, w.long_hint), dim3(RD_THREADS), 0, stream, in, w, n);
        const uint32_t grid = std::min<uint32_t>((n + RD_WAVES - 1) / RD_WAVES, (uint32_t)std::max(n_cu, 1) * 4u);
        hipLaunchKernelGGL(k_rd_long_measure, dim3(grid), dim3(RD_THREADS), 0, stream, in, table, w, n);
    }
    const uint32_t chunks = render_chunks(n);
    hipLaunchKernelGGL(k_rd_chunk_sum, dim3(chunks), dim3(RD_THREADS), 0, stream, (const uint64_t*)w.rec_len, n, w.chunk_sums);
    hipLaunchKernelGGL(k_rd_scan, dim3(chunks), dim3(RD_THREADS), 0, stream, (const uint64_t*)w.rec_len, n, (const uint64_t*)w.chunk_sums, w.rec_off, w.ctr, max_bytes);
    return hipGetLastError();
}

hipError_t render_write(const RenderInput& in, const PayloadTable& table, const RenderWork& w, uint8_t* text, uint64_t capacity, int n_cu, hipStream_t stream) {
    bool ok;
    const uint32_t n = record_count(in, ok);
    if (!ok) return hipErrorInvalidValue;
    if (!n || !capacity) return hipSuccess;   // nothing may be stored; the demand is counted by render_measure
    (void)n_cu;
    if (reinterpret_cast<uintptr_t>(text) & 15u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_rd_write_short, dim3((n + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, stream, in, table, w, n, text, capacity);
    hipLaunchKernelGGL(k_rd_write_long, long_grid(n, w.long_hint), dim3(RD_THREADS), 0, stream, in, table, w, n, text, capacity);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ payload texts
static size_t env_size(const char* name, size_t dflt) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v ? (size_t)v : dflt;
}

PayloadTexts::PayloadTexts() : max_entries_(env_size("MATCHY_AMD_RENDER_PAYLOADS", (size_t)1 << 20)), first_slots_(2),
      pool_cap_(env_size("MATCHY_AMD_RENDER_PAYLOADS_POOL_BYTES", (size_t)64 << 10)) {
    const size_t want = std::min<size_t>(env_size("MATCHY_AMD_RENDER_PAYLOADS_SLOTS", 64), (size_t)1 << 30);
    while (first_slots_ < want) first_slots_ *= 2;   // a power of two, at least 2
}

uint32_t PayloadTexts::find(uint32_t data_off) const {
    if (slots_.empty()) return RENDER_KEY_EMPTY;
    const uint32_t n = (uint32_t)slots_.size();
    for (uint32_t s = payload_slot(data_off, n);; s = (s + 1u) & (n - 1u)) {   // at most half full: an empty slot ends the walk
        if (slots_[s].key == data_off) return s;
        if (slots_[s].key == RENDER_KEY_EMPTY) return RENDER_KEY_EMPTY;
    }
}

void PayloadTexts::place(const PayloadSlot& e) {
    const uint32_t n = (uint32_t)slots_.size();
    uint32_t s = payload_slot(e.key, n);
    while (slots_[s].key != RENDER_KEY_EMPTY) s = (s + 1u) & (n - 1u);
    slots_[s] = e;
}

void PayloadTexts::add(uint32_t data_off, const std::string& json) {
    if (pool_.size() + json.size() > 0xFFFFFFFFull) throw HipError{"render: the payload texts exceed 4 GiB"};
    if (2 * (entries_ + 1) > slots_.size()) {   // grow and place every entry again
        std::vector<PayloadSlot> old;
        old.swap(slots_);
        slots_.assign(old.empty() ? first_slots_ : old.size() * 2, PayloadSlot{RENDER_KEY_EMPTY, 0, 0, 0});
        for (const PayloadSlot& e : old) if (e.key != RENDER_KEY_EMPTY) place(e);
        if (!old.empty()) ++rehashes_;
    }
    place(PayloadSlot{data_off, (uint32_t)pool_.size(), (uint32_t)json.size(), 0});
    pool_.insert(pool_.end(), json.begin(), json.end());
    ++entries_;
}

void PayloadTexts::clear() {
    slots_.clear(); pool_.clear(); entries_ = 0;
}

void PayloadTexts::upload(hipStream_t stream) {
    // fresh buffers, then swap: a table is never changed under a kernel that may still read it (the caller has waited for the stream)
    DevBuf<PayloadSlot> s;
    DevBuf<uint8_t> p;
    if (pool_.size() > pool_cap_) { pool_cap_ = pool_.size() * 2; ++pool_regrows_; }   // the pool has room for what the next batches add
    s.alloc(slots_.size());
    p.alloc(pool_cap_);
    if (!slots_.empty()) MXY_HIP(hipMemcpyAsync(s.p, slots_.data(), slots_.size() * sizeof(PayloadSlot), hipMemcpyHostToDevice, stream));
    if (!pool_.empty()) MXY_HIP(hipMemcpyAsync(p.p, pool_.data(), pool_.size(), hipMemcpyHostToDevice, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    slots_dev_.swap(s);
    pool_dev_.swap(p);
}

// ------------------------------------------------------------------------------------------------ host driver
void NdjsonRender::arm(const RenderParams& p, hipStream_t stream) {
    params_ = p;
    if (params_.sources.empty()) params_.sources.push_back("\"-\"");
    params_.line_bases.resize(params_.sources.size(), 0);
    // members: the copies below read them when the stream gets there, and they stay as they are until the next arm()
    std::vector<RenderSource>& table = source_table_;
    std::string& text = source_text_;
    table.clear(); text.clear();
    for (const std::string& s : params_.sources) { table.push_back(RenderSource{(uint32_t)text.size(), (uint32_t)s.size()}); text += s; }
    if (sources_dev_.n < table.size()) { sources_dev_.alloc(table.size() + 64); line_bases_dev_.alloc(table.size() + 64); }
    if (source_text_dev_.n < text.size()) source_text_dev_.alloc(text.size() + 4096);
    MXY_HIP(hipMemcpyAsync(sources_dev_.p, table.data(), table.size() * sizeof(RenderSource), hipMemcpyHostToDevice, stream));
    MXY_HIP(hipMemcpyAsync(source_text_dev_.p, text.data(), text.size(), hipMemcpyHostToDevice, stream));
    MXY_HIP(hipMemcpyAsync(line_bases_dev_.p, params_.line_bases.data(), params_.line_bases.size() * 8, hipMemcpyHostToDevice, stream));
}

RenderWork NdjsonRender::work() const {
    RenderWork w{};
    w.rec_len = rec_len_.p; w.rec_off = rec_off_.p; w.chunk_sums = chunks_.p; w.long_list = long_list_.p;
    w.piece_len = piece_len_.p; w.piece_off = piece_off_.p; w.piece_cap = (uint32_t)piece_len_.n;
    w.miss_set = miss_set_.p; w.miss_set_slots = (uint32_t)miss_set_.n; w.miss_list = miss_list_.p; w.miss_cap = (uint32_t)miss_list_.n;
    w.long_hint = long_hint_;
    w.ctr = reinterpret_cast<RenderCounters*>(ctr_.p);
    w.miss = reinterpret_cast<RenderMissCounter*>(ctr_.p + sizeof(RenderCounters));
    return w;
}

// one run of the pass on the stream of the fetch: (measure + offsets,) write, and the counters into pinned memory
void NdjsonRender::queue_round(bool measure) {
    const RenderWork w = work();
    const PayloadTable t = texts_.view();
    if (measure) {
        if (timed_) MXY_HIP(hipEventRecord(ev_[0], stream_));
        MXY_HIP(hipMemsetAsync(ctr_.p, 0, ctr_.n, stream_));
        MXY_HIP(hipMemsetAsync(miss_set_.p, 0xFF, miss_set_.n * 4, stream_));
        MXY_HIP(render_measure(in_, t, w, max_bytes_, n_cu_, stream_));
    }
    if (timed_) MXY_HIP(hipEventRecord(ev_[1], stream_));
    MXY_HIP(render_write(in_, t, w, text_.p, text_.n, n_cu_, stream_));
    if (timed_) MXY_HIP(hipEventRecord(ev_[2], stream_));
    MXY_HIP(hipMemcpyAsync(pinned_.p, ctr_.p, ctr_.n, hipMemcpyDeviceToHost, stream_));
}

void NdjsonRender::resolve(RenderInput in, bool to_host, int n_cu, bool profile, hipStream_t stream) {
    auto grown = [](size_t n) { return n + n / 4 + 1024; };
    const uint32_t n = in.b.n_fin + in.b.n_c4;
    in.flags = params_.flags;
    in.sources = sources_dev_.p; in.source_text = source_text_dev_.p; in.line_bases = line_bases_dev_.p;
    if (!params_.per_segment) { in.n_segments = 0; in.seg_of_fin = in.seg_of_c4 = in.seg_line_base = nullptr; }
    in_ = in; to_host_ = to_host; n_cu_ = n_cu; stream_ = stream; timed_ = profile;
    if (!max_bytes_) max_bytes_ = env_size("MATCHY_AMD_RENDER_MAX_BYTES", (size_t)1 << 30);
    if (rec_len_.n < n || !rec_off_.p) { const size_t want = grown(n); rec_len_.alloc(want); rec_off_.alloc(want + 1); long_list_.alloc(want); }
    if (chunks_.n < render_chunks(n)) chunks_.alloc(render_chunks(n) + 64);
    if (!piece_len_.p) { piece_len_.alloc(4096); piece_off_.alloc(4096); }
    if (!miss_set_.p) miss_set_.alloc(1u << 14);
    if (!miss_list_.p) miss_list_.alloc(4096);
    if (!ctr_.p) ctr_.alloc(sizeof(RenderCounters) + sizeof(RenderMissCounter));
    // the first block of a scanner: 256 bytes per record; afterwards what the scans before left
    if (!text_.n && n) text_.alloc((size_t)n * 256 + 4096);
    pinned_.ensure(ctr_.n);
    events_ = Events{};
    if (profile) for (Event& e : ev_) e.create();
    queue_round(true);
}

RenderView NdjsonRender::finish(PayloadFn payload, const void* ctx) {
    RenderView v;
    v.armed = true;
    const uint32_t n = in_.b.n_fin + in_.b.n_c4;
    uint32_t added_here = 0;   // payloads this batch brought into the table
    bool pieces_regrown = false;
    const bool trace = getenv("MATCHY_AMD_TRACE") != nullptr;
    const uint32_t rehashes0 = texts_.rehashes(), regrows0 = texts_.pool_regrows();
    std::string json;
    std::vector<uint32_t> list;
    for (;;) {
        const RenderCounters c = *reinterpret_cast<const RenderCounters*>(pinned_.p);
        const uint32_t misses = reinterpret_cast<const RenderMissCounter*>(pinned_.p + sizeof(RenderCounters))->misses;
        if (timed_) { MXY_HIP(hipEventElapsedTime(&ms_[0], ev_[0], ev_[1])); MXY_HIP(hipEventElapsedTime(&ms_[1], ev_[1], ev_[2])); }
        events_.misses += misses;
        bool again = false;
        long_hint_ = c.n_long;
        if (c.pieces_short) {
            // The piece arrays were too small. Their demand is counted (in 64 bits) and does not depend on the payload table, so one
            // regrow settles it: a second shortfall ends the pass. All but two pieces of a record are whole, and a whole piece is at
            // least RENDER_PIECE bytes of text: where that alone exceeds the limit nothing is allocated.
            const uint64_t whole = c.n_pieces > 2ull * c.n_long ? c.n_pieces - 2ull * c.n_long : 0;
            if (pieces_regrown || whole * RENDER_PIECE > max_bytes_ || c.n_pieces > 0xFFFF0000ull) { v.status = RENDER_TOO_LARGE; break; }
            if (trace) fprintf(stderr, "[matchy_amd] render: list pieces overflow: capacity %zu, need %llu\n", piece_len_.n, (unsigned long long)c.n_pieces);
            piece_len_.alloc((size_t)c.n_pieces + c.n_pieces / 4 + 1024); piece_off_.alloc(piece_len_.n);
            pieces_regrown = true;
            again = true;
        }
        if (misses > miss_list_.n) {   // the list overflowed: nothing of it is used, a longer one and a set to match
            if (trace) fprintf(stderr, "[matchy_amd] render: list miss_list overflow: capacity %zu, need %u\n", miss_list_.n, misses);
            miss_list_.alloc((size_t)misses + misses / 4 + 1024);
            size_t slots = miss_set_.n;
            while (slots < 4 * (size_t)misses && slots < ((size_t)1 << 22)) slots *= 2;
            if (slots != miss_set_.n) miss_set_.alloc(slots);
            again = true;
        } else if (misses) {
            list.resize(misses);
            MXY_HIP(hipMemcpyAsync(list.data(), miss_list_.p, (size_t)misses * 4, hipMemcpyDeviceToHost, stream_));
            MXY_HIP(hipStreamSynchronize(stream_));
            uint32_t fresh = 0;
            for (uint32_t off : list) {
                if (texts_.has(off)) continue;   // listed twice (a crowded set)
                if (texts_.entries() >= texts_.max_entries()) {
                    // bounded: emptied and refilled from the batch at hand, which finds its other payloads missing in the next round
                    if (added_here >= texts_.max_entries()) { v.status = RENDER_TOO_LARGE; break; }
                    texts_.clear();
                }
                payload(ctx, off, json);
                texts_.add(off, json);
                ++fresh; ++added_here;
            }
            if (v.status != RENDER_OK) break;
            // every repeat publishes at least one payload, or the loop ends here
            if (!fresh) throw HipError{"render: the pass reports payloads missing that the table holds"};
            events_.payloads_added += fresh;
            texts_.upload(stream_);
            again = true;
        }
        if (!again) { v.status = c.status; v.len = c.demand; break; }
        ++events_.rounds;
        queue_round(true);
        MXY_HIP(hipStreamSynchronize(stream_));
    }
    events_.copied = 0;
    events_.rehashes = texts_.rehashes() - rehashes0; events_.pool_regrows = texts_.pool_regrows() - regrows0;
    ms_[2] = 0;
    if (v.status != RENDER_OK || !n) { v.len = v.status == RENDER_OK ? v.len : 0; return v; }
    if (v.len > text_.n) {   // the block was too small: the demand is exact, so one regrow settles it, and only the write step runs again
        text_.alloc((size_t)v.len + v.len / 4 + 4096);
        queue_round(false);
        MXY_HIP(hipStreamSynchronize(stream_));
        if (timed_) MXY_HIP(hipEventElapsedTime(&ms_[1], ev_[1], ev_[2]));
    }
    if (to_host_ && v.len) {
        pinned_text_.ensure(v.len, v.len / 4 + (1 << 16));
        if (timed_) MXY_HIP(hipEventRecord(ev_[3], stream_));
        MXY_HIP(hipMemcpyAsync(pinned_text_.p, text_.p, v.len, hipMemcpyDeviceToHost, stream_));
        if (timed_) MXY_HIP(hipEventRecord(ev_[4], stream_));
        MXY_HIP(hipStreamSynchronize(stream_));
        if (timed_) MXY_HIP(hipEventElapsedTime(&ms_[2], ev_[3], ev_[4]));
        events_.copied = v.len;
        v.text = pinned_text_.p;
    } else v.text = v.len ? text_.p : nullptr;
    return v;
}

}  // namespace mxy
