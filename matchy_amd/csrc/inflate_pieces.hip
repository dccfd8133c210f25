// gz scans, pieces of one stream: one large member is inflated by many waves (the rules, and why a complete chain is the sequential
// parse of the stream: inflate_core.h "pieces of one stream"). Between the copy of the compressed bytes and the seal, on the scan's stream:
//   k_gz_piece_find      one wave per piece: 64 bit offsets per turn through the cheap test, survivors through read_dynamic by lane 0,
//                        in order; the first that parses is the piece's start. At most 8 * piece_bytes offsets.
//   k_gz_piece_count     one wave per piece that has a start: lane 0 runs the piece decoder dry and writes end bit, landing, bytes, status.
//   k_gz_piece_chain     one wave per split member: lane 0 walks the chain (at most n_pieces turns), writes out_pos and the live flags and
//                        whether the chain is complete.
//   k_gz_piece_symbols   one wave per live piece of a complete member: the piece decoder again, the wave executes the tokens into the
//                        member's 16-bit symbols at out_pos, like k_gz_inflate executes them into text. The count pass has fixed the
//                        piece's range [out_pos, out_pos + produced): every store is behind a test against it.
//   k_gz_piece_windows   one wave per split member, live pieces in chain order: the last min(32 768, produced) symbols of each piece
//                        become bytes of the text.
//   k_gz_piece_resolve   one wave per live piece: the rest of its symbols become bytes; CRC-32 of the piece times x^(8 * bytes behind it),
//                        xored into the member's word.
//   k_gz_piece_verdict   one wave: a member whose chain is complete, whose markers all resolved and whose CRC is the trailer's is OK;
//                        every other split member goes onto the handover list, which k_gz_inflate (inflate.hip) takes as its order list in
//                        a second launch: the member's status, and its precedence, are the one-wave path's.
// Bounds. Loads of compressed bytes go through the bit reader (behind the member's end) or the stored-run test here. A piece decoder
// consumes at least one bit per token: 8 * body_len + 2 turns at most, and it ends at the member's end, at its capacity, or once it has
// passed GZ_PIECE_MAX_SKIP candidates. No wave waits for another wave; what a later pass needs comes from an earlier launch.
// Stream windows (the second half of this file): the same passes over one window of a stream that is larger than a batch, with an open
// chain and the history of the text in front in place of a member's first byte.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "inflate.h"
#include "inflate_core.h"

namespace mxy {

namespace {

constexpr uint32_t GZ_PIECE_MAX_GRID = 65535;
static_assert(sizeof(gz::Tables) + gz::GZ_PIECE_QUEUE * sizeof(gz::Token) + 1024 + sizeof(gz::Batch) + 16 <= 3 * 1280, "three LDS granules per wave");

// As in inflate.hip: orders this wave's global stores in front of its later global loads; the wait is what the ordering rests on.
__device__ __forceinline__ void d_own_stores_visible() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The member of piece pi and the piece's index in it; false where the tables do not fit each other or the buffers (the host has
// planned them; these tests keep every access inside the buffers whatever they hold).
__device__ bool d_piece_member(const GzPieceArgs& a, uint32_t pi, GzMemberDev& m, uint32_t& idx) {
    const uint32_t mi = a.pieces[pi].member;
    if (mi >= a.n_members) return false;
    m = a.members[mi];
    const uint32_t first = m.reserved[1], n = m.reserved[2];
    if (pi < first || pi - first >= n || first > a.n_pieces || n > a.n_pieces - first) return false;
    if (m.body > a.packed_len || m.body_len > a.packed_len - m.body || m.start > a.text_len || m.cap > a.text_len - m.start) return false;
    idx = pi - first;
    return true;
}

// The first bit offset in [lo, hi) where a dynamic block header parses, by one wave: 64 offsets per turn through the cheap test, the
// survivors through read_dynamic by lane 0, in order. At most (hi - lo) / 64 + 1 turns of 64 offsets; every branch around a barrier
// depends on the ballot and the LDS word only. tab and hit are the wave's LDS.
__device__ __forceinline__ uint64_t d_find_start(const uint8_t* in, uint32_t in_len, uint64_t lo, uint64_t hi, gz::Tables& tab, uint32_t& hit, uint32_t lane) {
    uint64_t start = gz::GZ_PIECE_NO_START;
    for (uint64_t base = lo; base < hi && start == gz::GZ_PIECE_NO_START; base += 64u) {
        const uint64_t bit = base + lane;
        unsigned long long alive = __ballot(bit < hi && gz::piece_probe_cheap(in, in_len, bit));
        while (alive) {   // <= 64 turns, in stream order: the first that parses
            const uint32_t j = (uint32_t)__ffsll(alive) - 1u;
            alive &= alive - 1ull;
            __syncthreads();
            if (lane == 0) hit = gz::piece_probe(in, in_len, base + j, tab) ? 1u : 0u;
            __syncthreads();
            if (hit) { start = base + j; break; }
        }
    }
    return start;
}

__global__ __launch_bounds__(64) void k_gz_piece_find(GzPieceArgs a) {
    __shared__ gz::Tables tab;
    __shared__ uint32_t hit;
    const uint32_t lane = threadIdx.x;
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        GzMemberDev m;
        uint32_t idx;
        if (!d_piece_member(a, pi, m, idx)) continue;
        const uint8_t* in = a.packed + m.body;
        const uint64_t lo = (uint64_t)idx * a.piece_bytes * 8u, total = (uint64_t)m.body_len * 8u;
        const uint64_t hi = min(lo + (uint64_t)a.piece_bytes * 8u, total);
        const uint64_t start = idx ? d_find_start(in, m.body_len, lo, hi, tab, hit, lane) : 0ull;
        if (lane == 0) {
            a.starts[pi] = start;
            a.pieces[pi].start_bit = start == gz::GZ_PIECE_NO_START ? 0ull : start;
            a.pieces[pi].flags = start == gz::GZ_PIECE_NO_START ? 0u : gz::PIECE_HAS_START;
        }
    }
}

__global__ __launch_bounds__(64) void k_gz_piece_count(GzPieceArgs a) {
    __shared__ gz::Tables tab;
    __shared__ gz::Token queue[gz::GZ_PIECE_QUEUE];
    if (threadIdx.x != 0) return;   // no barrier below: the dry run is lane 0's alone
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        GzMemberDev m;
        uint32_t idx;
        if (!d_piece_member(a, pi, m, idx) || !(a.pieces[pi].flags & gz::PIECE_HAS_START)) continue;
        gz::PieceDecoder p;
        gz::piece_decoder_init(p, a.packed + m.body, m.body_len, m.cap, a.starts + m.reserved[1], m.reserved[2], idx, a.starts[pi]);
        gz::Batch batch;
        bool over = false;
        for (uint64_t turns = 8ull * m.body_len + 2ull; turns && !over; --turns) {
            gz::piece_decode_batch(p, tab, queue, gz::GZ_PIECE_QUEUE, batch);
            over = p.d.done || p.d.status != gz::GZ_OK;
        }
        int32_t st = over ? p.d.status : (int32_t)gz::GZ_TRUNCATED;
        if (st == gz::GZ_OK && p.landed == gz::GZ_PIECE_NONE) st = gz::GZ_PIECE_NO_LANDING;
        gz::Piece& pc = a.pieces[pi];
        pc.end_bit = p.end_bit; pc.next = p.landed; pc.produced = p.d.produced; pc.status = st;
    }
}

__global__ __launch_bounds__(64) void k_gz_piece_chain(GzPieceArgs a) {
    if (threadIdx.x != 0) return;
    for (uint32_t s = blockIdx.x; s < a.n_split; s += gridDim.x) {
        const uint32_t mi = a.split[s];
        if (mi >= a.n_members) continue;
        const GzMemberDev m = a.members[mi];
        const uint32_t first = m.reserved[1], n = m.reserved[2];
        bool ok = n != 0 && first <= a.n_pieces && n <= a.n_pieces - first && m.body <= a.packed_len && m.body_len <= a.packed_len - m.body;
        if (ok) ok = gz::piece_chain(a.pieces + first, n, a.packed + m.body, m.body_len, m.cap);
        a.complete[mi] = ok ? 1u : 0u;
    }
}

// The live piece pi of a complete member: its member, and its range of the scratch (inside scratch[0, scratch_len)).
__device__ bool d_live_piece(const GzPieceArgs& a, uint32_t pi, GzMemberDev& m, uint32_t& idx, gz::Piece& pc) {
    if (!d_piece_member(a, pi, m, idx)) return false;
    pc = a.pieces[pi];
    if (!(pc.flags & gz::PIECE_LIVE) || !a.complete[pc.member]) return false;
    if (pc.out_pos > m.cap || pc.produced > m.cap - pc.out_pos) return false;
    return (uint64_t)pc.sym_base + m.cap <= a.scratch_len;
}

// One live piece into its symbols, by one wave: lane 0 runs the decoder p (initialised by every lane alike), the wave executes the tokens
// into sym[0, own), the piece's own range of the scratch as the count pass has fixed it: every store is behind a test against it. A match
// may reach p.window bytes in front of the piece: those become markers. tab, queue, batch and ctl are the wave's LDS.
__device__ __forceinline__ void d_piece_symbols(gz::PieceDecoder& p, const uint8_t* in, uint32_t in_len, uint16_t* sym, uint32_t own, gz::Tables& tab, gz::Token* queue,
                                                gz::Batch& batch, uint32_t* ctl, uint32_t lane) {
    const uint32_t window = p.window;
    for (uint64_t turns = 8ull * in_len + 2ull; turns; --turns) {
        __syncthreads();   // the queue and the control word are free
        if (lane == 0) {
            gz::piece_decode_batch(p, tab, queue, gz::GZ_PIECE_QUEUE, batch);
            ctl[0] = (p.d.done || p.d.status != gz::GZ_OK || turns == 1ull) ? 1u : 0u;
        }
        __syncthreads();
        const uint32_t nq = min(batch.n, gz::GZ_PIECE_QUEUE);
        bool is_match = false;
        if (lane < nq) {
            const gz::Token t = queue[lane];
            is_match = gz::token_is_match(t);
            if (!is_match && t.pos < own) sym[t.pos] = (uint16_t)(t.v & 255u);
        }
        unsigned long long matches = __ballot(is_match);
        while (matches) {   // <= 64 turns, in stream order: a match may copy from the one in front of it
            const uint32_t j = (uint32_t)__ffsll(matches) - 1u;
            matches &= matches - 1ull;
            const gz::Token t = queue[j];
            const uint32_t len = gz::token_len(t), dist = gz::token_dist(t), pos = t.pos;
            d_own_stores_visible();
            if (dist == 0 || pos > own || len > own - pos || (dist > pos && dist - pos > window)) continue;   // piece_decode_batch hands no such token out
            for (uint32_t i = lane; i < len; i += 64u) {   // sources lie in front of pos: no stride reads what another writes
                const int32_t src = gz::piece_match_src(pos, dist, i);
                sym[pos + i] = src >= 0 ? sym[src] : (uint16_t)(gz::GZ_SYM_MARKER + (uint32_t)(-1 - src));
            }
        }
        const uint32_t sl = batch.stored_len, ss = batch.stored_src, sp = batch.stored_pos;
        if (sl && ss <= in_len && sl <= in_len - ss && sp <= own && sl <= own - sp)
            for (uint32_t i = lane; i < sl; i += 64u) sym[sp + i] = in[ss + i];
        if (ctl[0]) break;
    }
}

__global__ __launch_bounds__(64) void k_gz_piece_symbols(GzPieceArgs a) {
    __shared__ gz::Tables tab;
    __shared__ gz::Token queue[gz::GZ_PIECE_QUEUE];
    __shared__ gz::Batch batch;
    __shared__ uint32_t ctl[2];
    const uint32_t lane = threadIdx.x;
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        GzMemberDev m;
        uint32_t idx;
        gz::Piece pc;
        if (!d_live_piece(a, pi, m, idx, pc)) continue;   // wave-uniform: every lane reads the same records
        gz::PieceDecoder p;   // lane 0's copy is the decoder
        gz::piece_decoder_init(p, a.packed + m.body, m.body_len, m.cap, a.starts + m.reserved[1], m.reserved[2], idx, a.starts[pi]);
        d_piece_symbols(p, a.packed + m.body, m.body_len, a.scratch + pc.sym_base + pc.out_pos, pc.produced, tab, queue, batch, ctl, lane);
    }
}

// Markers of piece i point into text[out_pos_i - 32768, out_pos_i). Induction over the chain: when the wave reaches piece i, those
// bytes are final. They are the last bytes of the pieces in front: the tail (the last min(32768, produced) bytes) of piece i - 1, and
// where that piece produced less than 32 KiB its tail is the whole piece and the range goes on into the tail of piece i - 2, and so on —
// every byte of the range lies in the tail of the piece that produced it, and the tails of all pieces in front have been written by
// this wave in chain order, each from symbols that are bytes or markers into a range that was final by the same argument (piece 0 has
// no markers: its decoder refuses a distance beyond its own bytes). The fence between two pieces puts the stores in front of the loads.
// A marker in front of the member's first byte ends the member here: it is handed over and the one-wave path names the error.
// STREAM (stream windows): a marker in front of the text's first byte reads history[0, history_len) (gz::stream_resolve_sym).
template <bool STREAM = false>
__device__ bool d_resolve(const uint16_t* sym, uint8_t* text, uint32_t out_pos, uint32_t from, uint32_t to, uint32_t lane, const uint8_t* history = nullptr,
                          uint32_t history_len = 0) {
    // eight symbols per lane and turn, all loads in front of the stores: a marker's byte lies in front of out_pos, so no load of a turn
    // depends on a store of it, and the wave keeps eight loads in flight where one symbol per turn waits for each (to < 2^31: no wrap)
    constexpr uint32_t UNROLL = 8;
    bool bad = false;
    for (uint32_t j0 = from + lane; j0 < to; j0 += 64u * UNROLL) {
        uint32_t s[UNROLL];
        uint8_t b[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) s[u] = j0 + 64u * u < to ? sym[out_pos + j0 + 64u * u] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            b[u] = (uint8_t)'\n';
            bad |= STREAM ? !gz::stream_resolve_sym(s[u], text, out_pos, history, history_len, b[u]) : !gz::piece_resolve_sym(s[u], text, out_pos, b[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) if (j0 + 64u * u < to) text[out_pos + j0 + 64u * u] = b[u];
    }
    return __ballot(bad) != 0;
}

__global__ __launch_bounds__(64) void k_gz_piece_windows(GzPieceArgs a) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < a.n_split; s += gridDim.x) {
        const uint32_t mi = a.split[s];
        if (mi >= a.n_members || !a.complete[mi]) continue;
        const uint32_t first = a.members[mi].reserved[1], n = a.members[mi].reserved[2];
        for (uint32_t k = 0; k < n; ++k) {   // index order is chain order
            GzMemberDev m;
            uint32_t idx;
            gz::Piece pc;
            if (first + k >= a.n_pieces || !d_live_piece(a, first + k, m, idx, pc)) continue;
            const uint32_t tail = min(pc.produced, gz::GZ_PIECE_WINDOW);
            const bool bad = d_resolve(a.scratch + pc.sym_base, a.text + m.start, pc.out_pos, pc.produced - tail, pc.produced, lane);
            d_own_stores_visible();
            if (bad) { if (lane == 0) a.complete[mi] = 0; break; }
        }
    }
}

__global__ __launch_bounds__(64) void k_gz_piece_resolve(GzPieceArgs a) {
    __shared__ uint32_t crc_tab[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < 256u; k += 64u) crc_tab[k] = gz::crc_table_entry(k);
    __syncthreads();
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        GzMemberDev m;
        uint32_t idx;
        gz::Piece pc;
        if (!d_live_piece(a, pi, m, idx, pc)) continue;
        const uint32_t tail = min(pc.produced, gz::GZ_PIECE_WINDOW);
        uint8_t* text = a.text + m.start;
        if (d_resolve(a.scratch + pc.sym_base, text, pc.out_pos, 0, pc.produced - tail, lane)) { if (lane == 0) atomicExch(&a.failed[pc.member], 1u); continue; }
        d_own_stores_visible();
        uint32_t crc = gz::crc_lane_part(crc_tab, text + pc.out_pos, pc.produced, lane, 64u);
        for (int off = 32; off; off >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, off, 64);
        if (lane == 0) atomicXor(&a.crc[pc.member], gz::crc_mul(crc, gz::crc_xpow8(m.cap - pc.out_pos - pc.produced)));
    }
}

__global__ __launch_bounds__(64) void k_gz_piece_verdict(GzPieceArgs a, int32_t* __restrict__ status, uint32_t* __restrict__ handover) {
    __shared__ uint32_t n_handed;
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x != 0) return;
    if (lane == 0) n_handed = 0;
    __syncthreads();
    for (uint32_t s = lane; s < a.n_split; s += 64u) {
        const uint32_t mi = a.split[s];
        if (mi >= a.n_members) continue;
        const GzMemberDev m = a.members[mi];
        bool ok = a.complete[mi] != 0 && a.failed[mi] == 0;
        if (ok) {   // the chain has found exactly 8 bytes behind the last block
            const uint8_t* t = a.packed + m.body + m.body_len - 8u;
            ok = ((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24) == a.crc[mi];
        }
        if (ok) { status[mi] = gz::GZ_OK; continue; }
        handover[atomicAdd(&n_handed, 1u)] = mi;
        const uint32_t first = m.reserved[1], n = m.reserved[2];
        for (uint32_t k = 0; k < n && first + k < a.n_pieces; ++k) a.pieces[first + k].flags |= gz::PIECE_HANDED;
    }
    __syncthreads();
    for (uint32_t s = n_handed + lane; s < a.n_split; s += 64u) handover[s] = 0xFFFFFFFFu;   // k_gz_inflate skips an index that is no member
}

// ------------------------------------------------------------------------------------------------ stream windows
// One window of a DEFLATE stream that is larger than a batch (GzStreamArgs, inflate.h; the rules: inflate_core.h "windows of one
// stream"). The passes are those of a split member with an OPEN chain in the middle: the chain ends where the window's text is full or
// its bytes run out, and the verdict hands that bit on as the start of the next window.
//   k_gz_stream_find     as k_gz_piece_find; piece 0 starts at the state's bit.
//   k_gz_stream_count    as k_gz_piece_count; piece 0 may reach history_len bytes in front of itself.
//   k_gz_stream_chain    one lane: gz::stream_chain; out_pos, the live flags, and in *dev the live count, the text's length, the end bit
//                        and whether the stream ended.
//   k_gz_stream_symbols  as k_gz_piece_symbols, into scratch[out_pos, out_pos + produced) with out_pos + produced <= text_cap.
//   k_gz_stream_windows  one wave, live pieces in chain order: the induction of k_gz_piece_windows, which here starts from the history:
//                        piece 0 has markers too, and they point into bytes that were final before the launch.
//   k_gz_stream_resolve  as k_gz_piece_resolve; a piece's CRC times x^(8 * (text_len - out_pos - produced)), xored into dev->crc.
//   k_gz_stream_verdict  one workgroup: status, and for an OK window the state behind it — the new history is taken here, in front of the
//                        line tail, which overwrites the partial line — and '\n' over the batch behind the text; otherwise over all of it.
// Bounds. in[0, in_len) is the only range compressed bytes are loaded from (the bit reader, the stored-run test, stream_end_check);
// every symbol store is inside the piece's [out_pos, out_pos + produced), which d_stream_live tests against text_cap; every text store
// is below carry_len + text_cap < batch_len. Turn bounds are those of the member kernels.
__device__ bool d_stream_live(const GzStreamArgs& a, uint32_t pi, gz::Piece& pc, uint32_t& text_len) {
    if (a.dev->n_live == 0) return false;
    text_len = min(a.dev->text_len, a.text_cap);
    pc = a.pieces[pi];
    return (pc.flags & gz::PIECE_LIVE) && pc.out_pos <= text_len && pc.produced <= text_len - pc.out_pos;
}

__global__ __launch_bounds__(64) void k_gz_stream_find(GzStreamArgs a) {
    __shared__ gz::Tables tab;
    __shared__ uint32_t hit;
    const uint32_t lane = threadIdx.x;
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        const uint64_t lo = (uint64_t)pi * a.piece_bytes * 8u, total = (uint64_t)a.in_len * 8u;
        const uint64_t hi = min(lo + (uint64_t)a.piece_bytes * 8u, total);
        const uint64_t start = pi ? d_find_start(a.in, a.in_len, lo, hi, tab, hit, lane) : (uint64_t)(a.bit & 7u);
        if (lane == 0) {
            a.starts[pi] = start;
            a.pieces[pi].start_bit = start == gz::GZ_PIECE_NO_START ? 0ull : start;
            a.pieces[pi].flags = start == gz::GZ_PIECE_NO_START ? 0u : gz::PIECE_HAS_START;
        }
    }
}

__global__ __launch_bounds__(64) void k_gz_stream_count(GzStreamArgs a) {
    __shared__ gz::Tables tab;
    __shared__ gz::Token queue[gz::GZ_PIECE_QUEUE];
    if (threadIdx.x != 0) return;   // no barrier below: the dry run is lane 0's alone
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        if (!(a.pieces[pi].flags & gz::PIECE_HAS_START)) continue;
        gz::PieceDecoder p;
        gz::stream_piece_decoder_init(p, a.in, a.in_len, a.text_cap, a.starts, a.n_pieces, pi, a.starts[pi], a.history_len);
        gz::Batch batch;
        bool over = false;
        for (uint64_t turns = 8ull * a.in_len + 2ull; turns && !over; --turns) {
            gz::piece_decode_batch(p, tab, queue, gz::GZ_PIECE_QUEUE, batch);
            over = p.d.done || p.d.status != gz::GZ_OK;
        }
        int32_t st = over ? p.d.status : (int32_t)gz::GZ_TRUNCATED;
        if (st == gz::GZ_OK && p.landed == gz::GZ_PIECE_NONE) st = gz::GZ_PIECE_NO_LANDING;
        gz::Piece& pc = a.pieces[pi];
        pc.end_bit = p.end_bit; pc.next = p.landed; pc.produced = p.d.produced; pc.status = st;
    }
}

__global__ __launch_bounds__(64) void k_gz_stream_chain(GzStreamArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const gz::StreamChain c = gz::stream_chain(a.pieces, a.n_pieces, a.text_cap, a.file_end != 0);
    GzStreamDev& d = *a.dev;
    d.consumed_bits = c.consumed_bits; d.n_live = c.n_live; d.text_len = c.text_len; d.ended = c.ended ? 1u : 0u; d.chain_failed = c.failed;
}

__global__ __launch_bounds__(64) void k_gz_stream_symbols(GzStreamArgs a) {
    __shared__ gz::Tables tab;
    __shared__ gz::Token queue[gz::GZ_PIECE_QUEUE];
    __shared__ gz::Batch batch;
    __shared__ uint32_t ctl[2];
    const uint32_t lane = threadIdx.x;
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        gz::Piece pc;
        uint32_t text_len;
        if (!d_stream_live(a, pi, pc, text_len)) continue;   // wave-uniform: every lane reads the same records
        gz::PieceDecoder p;   // lane 0's copy is the decoder
        gz::stream_piece_decoder_init(p, a.in, a.in_len, a.text_cap, a.starts, a.n_pieces, pi, a.starts[pi], a.history_len);
        d_piece_symbols(p, a.in, a.in_len, a.scratch + pc.out_pos, pc.produced, tab, queue, batch, ctl, lane);
    }
}

__global__ __launch_bounds__(64) void k_gz_stream_windows(GzStreamArgs a) {
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x != 0) return;
    for (uint32_t k = 0; k < a.n_pieces; ++k) {   // index order is chain order
        gz::Piece pc;
        uint32_t text_len;
        if (!d_stream_live(a, k, pc, text_len)) continue;
        const uint32_t tail = min(pc.produced, gz::GZ_PIECE_WINDOW);
        const bool bad = d_resolve<true>(a.scratch, a.batch + a.carry_len, pc.out_pos, pc.produced - tail, pc.produced, lane, a.state->history, a.history_len);
        d_own_stores_visible();
        if (bad) { if (lane == 0) a.dev->bad = 1u; break; }
    }
}

__global__ __launch_bounds__(64) void k_gz_stream_resolve(GzStreamArgs a) {
    __shared__ uint32_t crc_tab[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < 256u; k += 64u) crc_tab[k] = gz::crc_table_entry(k);
    __syncthreads();
    for (uint32_t pi = blockIdx.x; pi < a.n_pieces; pi += gridDim.x) {
        gz::Piece pc;
        uint32_t text_len;
        if (!d_stream_live(a, pi, pc, text_len)) continue;
        const uint32_t tail = min(pc.produced, gz::GZ_PIECE_WINDOW);
        uint8_t* text = a.batch + a.carry_len;
        if (d_resolve<true>(a.scratch, text, pc.out_pos, 0, pc.produced - tail, lane, a.state->history, a.history_len)) { if (lane == 0) atomicExch(&a.dev->bad, 1u); continue; }
        d_own_stores_visible();
        uint32_t crc = gz::crc_lane_part(crc_tab, text + pc.out_pos, pc.produced, lane, 64u);
        for (int off = 32; off; off >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, off, 64);
        if (lane == 0) atomicXor(&a.dev->crc, gz::stream_piece_crc(crc, text_len, pc.out_pos, pc.produced));
    }
}

constexpr uint32_t GZ_STREAM_VERDICT_THREADS = 256;
__global__ __launch_bounds__(GZ_STREAM_VERDICT_THREADS) void k_gz_stream_verdict(GzStreamArgs a) {
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x != 0) return;
    // every thread reads the same words and takes the same branch; nothing below waits for another thread
    const GzStreamDev d = *a.dev;
    const uint32_t text_len = min(d.text_len, a.text_cap), history_len = min(a.history_len, gz::GZ_PIECE_WINDOW);
    int32_t status = gz::STREAM_OK, gz_status = gz::GZ_OK;
    uint32_t all_crc = 0;
    if (d.n_live == 0) { gz_status = d.chain_failed; status = gz_status != gz::GZ_OK ? gz::STREAM_FAILED : gz::STREAM_NO_PROGRESS; }
    else if (d.bad) { status = gz::STREAM_FAILED; gz_status = gz::GZ_BAD_DISTANCE; }
    else {
        all_crc = gz::stream_crc_combine(a.state->crc, d.crc, text_len);
        if (d.ended) gz_status = gz::stream_end_check(a.in, a.in_len, d.consumed_bits, a.state->text_bytes, text_len, all_crc);
        if (gz_status != gz::GZ_OK) status = gz::STREAM_FAILED;
    }
    const uint32_t keep = status == gz::STREAM_OK ? a.carry_len + text_len : 0u;   // <= carry_len + text_cap < batch_len
    if (status == gz::STREAM_OK) {
        const uint32_t new_len = gz::stream_history_len(history_len, text_len);
        const uint8_t* text = a.batch + a.carry_len;
        for (uint32_t j = tid; j < new_len; j += GZ_STREAM_VERDICT_THREADS)
            a.state_out->history[j] = gz::stream_history_byte(a.state->history, history_len, text, text_len, new_len, j);
        if (tid == 0) {
            a.state_out->text_bytes = a.state->text_bytes + text_len; a.state_out->crc = all_crc;
            a.state_out->bit = (uint32_t)(d.consumed_bits & 7u); a.state_out->history_len = new_len;
        }
    }
    for (uint32_t i = keep + tid; i < a.batch_len; i += GZ_STREAM_VERDICT_THREADS) a.batch[i] = (uint8_t)'\n';
    if (tid == 0) { a.dev->status = status; a.dev->gz_status = gz_status; }
}

template <class K, class... Args>
hipError_t launch_over(K kernel, uint32_t n, hipStream_t stream, Args... args) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(std::min(n, GZ_PIECE_MAX_GRID)), dim3(64), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace

hipError_t gz_piece_find_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_find, a.n_pieces, stream, a); }
hipError_t gz_piece_count_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_count, a.n_pieces, stream, a); }
hipError_t gz_piece_chain_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_chain, a.n_split, stream, a); }
hipError_t gz_piece_symbols_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_symbols, a.n_pieces, stream, a); }
hipError_t gz_piece_windows_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_windows, a.n_split, stream, a); }
hipError_t gz_piece_resolve_launch(const GzPieceArgs& a, hipStream_t stream) { return launch_over(k_gz_piece_resolve, a.n_pieces, stream, a); }
hipError_t gz_piece_verdict_launch(const GzPieceArgs& a, int32_t* status, uint32_t* handover, hipStream_t stream) {
    if (a.n_split == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gz_piece_verdict, dim3(1), dim3(64), 0, stream, a, status, handover);
    return hipGetLastError();
}

hipError_t gz_stream_find_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_find, a.n_pieces, stream, a); }
hipError_t gz_stream_count_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_count, a.n_pieces, stream, a); }
hipError_t gz_stream_chain_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_chain, a.n_pieces ? 1u : 0u, stream, a); }
hipError_t gz_stream_symbols_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_symbols, a.n_pieces, stream, a); }
hipError_t gz_stream_windows_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_windows, a.n_pieces ? 1u : 0u, stream, a); }
hipError_t gz_stream_resolve_launch(const GzStreamArgs& a, hipStream_t stream) { return launch_over(k_gz_stream_resolve, a.n_pieces, stream, a); }
hipError_t gz_stream_verdict_launch(const GzStreamArgs& a, hipStream_t stream) {
    if (a.n_pieces == 0 || a.batch_len == 0 || a.carry_len > a.batch_len || a.text_cap >= a.batch_len - a.carry_len) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gz_stream_verdict, dim3(1), dim3(GZ_STREAM_VERDICT_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace mxy
