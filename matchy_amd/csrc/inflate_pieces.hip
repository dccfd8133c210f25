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
        uint64_t start = idx ? gz::GZ_PIECE_NO_START : 0ull;
        // at most piece_bytes / 8 turns of 64 offsets; every branch around a barrier depends on the ballot and the LDS word only
        for (uint64_t base = lo; idx && base < hi && start == gz::GZ_PIECE_NO_START; base += 64u) {
            const uint64_t bit = base + lane;
            unsigned long long alive = __ballot(bit < hi && gz::piece_probe_cheap(in, m.body_len, bit));
            while (alive) {   // <= 64 turns, in stream order: the first that parses
                const uint32_t j = (uint32_t)__ffsll(alive) - 1u;
                alive &= alive - 1ull;
                __syncthreads();
                if (lane == 0) hit = gz::piece_probe(in, m.body_len, base + j, tab) ? 1u : 0u;
                __syncthreads();
                if (hit) { start = base + j; break; }
            }
        }
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
        const uint8_t* in = a.packed + m.body;
        uint16_t* sym = a.scratch + pc.sym_base + pc.out_pos;
        const uint32_t own = pc.produced, window = idx ? gz::GZ_PIECE_WINDOW : 0u;
        gz::PieceDecoder p;   // lane 0's copy is the decoder
        gz::piece_decoder_init(p, in, m.body_len, m.cap, a.starts + m.reserved[1], m.reserved[2], idx, a.starts[pi]);
        for (uint64_t turns = 8ull * m.body_len + 2ull; turns; --turns) {
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
            if (sl && ss <= m.body_len && sl <= m.body_len - ss && sp <= own && sl <= own - sp)
                for (uint32_t i = lane; i < sl; i += 64u) sym[sp + i] = in[ss + i];
            if (ctl[0]) break;
        }
    }
}

// Markers of piece i point into text[out_pos_i - 32768, out_pos_i). Induction over the chain: when the wave reaches piece i, those
// bytes are final. They are the last bytes of the pieces in front: the tail (the last min(32768, produced) bytes) of piece i - 1, and
// where that piece produced less than 32 KiB its tail is the whole piece and the range goes on into the tail of piece i - 2, and so on —
// every byte of the range lies in the tail of the piece that produced it, and the tails of all pieces in front have been written by
// this wave in chain order, each from symbols that are bytes or markers into a range that was final by the same argument (piece 0 has
// no markers: its decoder refuses a distance beyond its own bytes). The fence between two pieces puts the stores in front of the loads.
// A marker in front of the member's first byte ends the member here: it is handed over and the one-wave path names the error.
__device__ bool d_resolve(const uint16_t* sym, uint8_t* text, uint32_t out_pos, uint32_t from, uint32_t to, uint32_t lane) {
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
        for (uint32_t u = 0; u < UNROLL; ++u) { b[u] = (uint8_t)'\n'; bad |= !gz::piece_resolve_sym(s[u], text, out_pos, b[u]); }
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

}  // namespace mxy
