// Percent- and JSON-escaped inputs, decoded on the GPU in front of the scan. The rules are unescape_core.h (decode() of a position from
// a Window: a lane's 16 bytes, 6 in front, 11 behind, and their esc bits); this file is the steps over tiles of TILE_BYTES input bytes, one
// wave per tile, lane l on bytes 16 l .. 16 l + 15:
//   k_unesc_count   output bytes of every tile. The bytes across a lane boundary come from cross-lane moves, those across the tile's
//                   boundaries from one 8-byte load in front (lane 0) and one 16-byte load behind (lane 63). The escapes, U+FFFD and LF
//                   escapes are summed per wave and added to the counter block.
//   prefix          exclusive prefix over the tiles: the kernels of the line index (tile_prefix_build); k_unesc_seal puts the total into
//                   the counter block.
//   k_unesc_write   a wave stages its tile's output in LDS (at most TILE_OUT_MAX bytes) — each lane at the exclusive wave scan of its
//                   lengths — and stores the part of the tile's output range that covers whole 16-byte lines of the text as 16-byte
//                   stores; the ragged head and tail share lines with the neighbouring tiles and go out as byte stores. Every output
//                   byte is written by exactly one lane, and no kernel reads the text.
// A full tile without a '%' (PERCENT) or '\\' (JSON) byte in it or in the 2 (5) bytes in front of it — no escape reaches into it, and it
// is not entered in the escaped state — takes a fast path in both kernels: its length is TILE_BYTES and its staged bytes are its own. In
// the other tiles a lane without such a byte in reach copies its bytes. The store phase is shared, so the text is the same either way.
// No load reaches data + len (the ragged end is read byte by byte), and nothing is stored without a bound that follows from the prefix.
//
// The escape state at a tile's first byte (JSON only; PERCENT launches none of this). Chosen: a small code pass and a two-level scan in
// front of count, not a count step that records both variants. The count and write steps are the dear ones — they decode — and this way
// each decodes every tile once, with its state known, and the prefix step stays the line index's; the code pass reads 16 bytes per
// tile, which is 1/64 of the batch, and the scan 4 bytes per tile.
//   k_unesc_code    one lane per full tile reads the tile's last 16 bytes. A byte other than '\\' among the first ten of them fixes esc
//                   of everything behind it, and the tile's code (tail_code) follows from those 16 bytes alone. Otherwise the wave reads
//                   the tile once, 16 bytes a lane, and one ballot finds where the backslash run begins: work is bounded by the tile,
//                   so a batch of backslashes costs one more read of itself and nothing quadratic.
//   k_unesc_chunk   the codes of UNESCAPE_STATE_CHUNK tiles, composed in order (fn_compose) -> one function per chunk
//   k_unesc_scan    one workgroup per chunk: the functions of the chunks in front of it, composed; then an ordered scan over its own
//                   tiles; state[t + 1] = code[t] applied to state[t].
// No workgroup waits for another one's store: the three are separate launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>

#include "unescape.h"

namespace mxy {

namespace {

using namespace unescape;

constexpr uint32_t UE_THREADS = 256, UE_WAVES = UE_THREADS / 64;
// a 16-byte store is put together from five dwords of the stage: the last one may begin 12 bytes in front of the end of the output.
// A multiple of 16, so that every wave's stage is aligned for the 16-byte stores of the fast path.
constexpr uint32_t STAGE_BYTES = (TILE_OUT_MAX + 16 + 15) / 16 * 16;
static_assert(TILE_BYTES == 64 * 16 && LANE_BYTES == 16 && TILE_LANES == 64, "a tile is one 16-byte load of every lane of a wave");
static_assert(STAGE_BYTES >= TILE_OUT_MAX + 16 && STAGE_BYTES >= TILE_BYTES, "the stage holds the longest output of a tile and the five dwords of its last store");
static_assert(LOOK_BEHIND <= 8 && LOOK_AHEAD <= 12, "the bytes across a tile's boundaries: one 8-byte load in front, three dwords behind");
constexpr uint32_t STATE_ITEMS = UNESCAPE_STATE_CHUNK / UE_THREADS;
static_assert(STATE_ITEMS * UE_THREADS == UNESCAPE_STATE_CHUNK, "a thread of the state scan owns STATE_ITEMS consecutive tiles");

// 16 bytes at `off` (a multiple of 16; `data` is 16-byte aligned); bytes at or behind `len` read as zero and are not touched
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 16u <= len) return *reinterpret_cast<const uint4*>(data + off);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16u; ++k)
        if (off + k < len) w[k >> 2] |= (uint32_t)data[off + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ bool has_byte(uint32_t x, uint32_t c) {   // one of the four bytes of x is c
    const uint32_t v = x ^ (c * 0x01010101u);
    return ((v - 0x01010101u) & ~v & 0x80808080u) != 0u;
}
__device__ __forceinline__ uint32_t byte_of(uint32_t x, uint32_t k) { return (x >> (8u * k)) & 0xFFu; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (uint32_t off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, uint32_t lane) {
    uint32_t incl = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    return incl - v;
}
// backslashes at the end of a lane's 16 bytes (bs: bit k = byte k is one)
__device__ __forceinline__ uint32_t trailing_run(uint32_t bs) { return (uint32_t)__clz((int)~(bs << 16)); }   // ~(..) has its low 16 bits set

// The window of lane `lane` of tile t (t * TILE_BYTES < len) and `raw`, the lane's 16 bytes. Returns true, with `w` untouched, when
// the tile takes the fast path; the answer is the same in every lane. `literal`: every position of the lane emits itself. state: the
// tile's (JSON), 0 otherwise. All 64 lanes call it.
template <uint32_t MODE>
__device__ __forceinline__ bool lane_window(const uint8_t* __restrict__ data, uint32_t len, uint32_t t, uint32_t lane, uint32_t state, Window& w, uint4& raw,
                                            bool& literal) {
    constexpr uint32_t C = MODE == MODE_JSON ? '\\' : '%';
    const uint32_t ts = t * TILE_BYTES, off = ts + lane * LANE_BYTES;   // below 2^31 + TILE_BYTES
    raw = off < len ? load16(data, off, len) : make_uint4(0, 0, 0, 0);
    uint2 front = make_uint2(0, 0);   // lane 0: the eight bytes in front of the tile
    if (lane == 0 && t != 0) front = *reinterpret_cast<const uint2*>(data + ts - 8u);
    bool opens = has_byte(raw.x, C) || has_byte(raw.y, C) || has_byte(raw.z, C) || has_byte(raw.w, C);
    // an escape that begins in front of the tile reaches into it from at most 5 (JSON) or 2 (PERCENT) bytes away
    opens = opens || (MODE == MODE_JSON ? has_byte(front.x & 0xFF000000u, C) || has_byte(front.y, C) : has_byte(front.y & 0xFFFF0000u, C));
    if (__ballot(opens) == 0ull && ts + TILE_BYTES <= len) return true;
    uint4 edge = make_uint4(0, 0, 0, 0);   // lane 63: the bytes behind the tile
    if (lane == 63 && ts + TILE_BYTES < len) edge = load16(data, ts + TILE_BYTES, len);
    uint32_t pz = __shfl_up(raw.z, 1), pw = __shfl_up(raw.w, 1);
    uint32_t nx = __shfl_down(raw.x, 1), ny = __shfl_down(raw.y, 1), nz = __shfl_down(raw.z, 1);
    if (lane == 0) { pz = front.x; pw = front.y; }
    if (lane == 63) { nx = edge.x; ny = edge.y; nz = edge.z; }
    const bool has_front = off != 0;   // then all six bytes in front exist: off >= 16
    const uint32_t own[4] = {raw.x, raw.y, raw.z, raw.w}, next[3] = {nx, ny, nz};
#pragma unroll
    for (uint32_t j = 0; j < LOOK_BEHIND; ++j) w.b[j] = has_front ? (j < 2u ? byte_of(pz, j + 2u) : byte_of(pw, j - 2u)) : BYTE_NONE;
#pragma unroll
    for (uint32_t k = 0; k < LANE_BYTES; ++k) w.b[OWN + k] = off + k < len ? byte_of(own[k >> 2], k & 3u) : BYTE_NONE;
#pragma unroll
    for (uint32_t k = 0; k < LOOK_AHEAD; ++k) w.b[OWN + LANE_BYTES + k] = off + LANE_BYTES + k < len ? byte_of(next[k >> 2], k & 3u) : BYTE_NONE;
    w.esc = 0;
    if (MODE == MODE_JSON) {
        // esc of the lane's first byte: the parity of the backslash run at the end of the nearest lane below that is not all
        // backslashes (a whole lane of them is an even run), or the tile's state where there is none
        uint32_t bs = 0;
#pragma unroll
        for (uint32_t k = 0; k < LANE_BYTES; ++k) bs |= (uint32_t)(w.b[OWN + k] == '\\') << k;
        const uint32_t run = trailing_run(bs);
        const uint64_t broken = __ballot(run != LANE_BYTES), odd = __ballot(run & 1u);
        const uint64_t below = broken & ((1ull << lane) - 1ull);
        const uint32_t e_in = below ? (uint32_t)((odd >> (63 - __clzll((long long)below))) & 1ull) : (state & 1u);
        const uint32_t mine = lane_esc(w, e_in);
        const uint32_t prev = __shfl_up(mine, 1);
        w.esc = (lane == 0 ? (state >> 1) & 0x3Fu : (prev >> (LANE_BYTES - LOOK_BEHIND)) & 0x3Fu) | (mine << OWN);
    }
    literal = lane_is_literal(w, MODE);
    return false;
}

// bytes of the input a lane has
__device__ __forceinline__ uint32_t lane_valid(uint32_t len, uint32_t t, uint32_t lane) {
    const uint32_t off = t * TILE_BYTES + lane * LANE_BYTES;
    return off < len ? min(len - off, LANE_BYTES) : 0u;
}

template <uint32_t MODE>
__global__ __launch_bounds__(UE_THREADS) void k_unesc_count(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, const uint8_t* __restrict__ state,
                                                            uint32_t* __restrict__ counts, UnescapeCounters* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * UE_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * UE_WAVES;
    uint32_t escapes = 0, replaced = 0, lfs = 0;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        Window w;
        uint4 raw;
        bool literal;
        uint32_t total = TILE_BYTES;
        if (!lane_window<MODE>(data, len, t, lane, MODE == MODE_JSON ? state[t] : 0u, w, raw, literal)) {
            uint32_t mine = lane_valid(len, t, lane);
            if (!literal) {
                mine = 0;
#pragma unroll
                for (uint32_t k = 0; k < LANE_BYTES; ++k) {
                    const Item it = decode(w, OWN + k, MODE);
                    mine += it.len;
                    escapes += it.flags & F_ESCAPE ? 1u : 0u;
                    replaced += it.flags & F_REPLACED ? 1u : 0u;
                    lfs += it.flags & F_LF ? 1u : 0u;
                }
            }
            total = wave_sum(mine);
        }
        if (lane == 0) counts[t] = total;
    }
    escapes = wave_sum(escapes); replaced = wave_sum(replaced); lfs = wave_sum(lfs);
    if (lane == 0) {
        if (escapes) atomicAdd(&ctr->escapes, escapes);
        if (replaced) atomicAdd(&ctr->replaced, replaced);
        if (lfs) atomicAdd(&ctr->lf_escapes, lfs);
    }
}

__global__ void k_unesc_seal(const uint32_t* __restrict__ prefix, uint32_t n_tiles, UnescapeCounters* __restrict__ ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctr->text_len = prefix[n_tiles];
}

// The waves of a workgroup take the same number of rounds (a wave without a tile in the last round idles through it), so the barriers
// between the stage's writers and readers are met by all of them.
template <uint32_t MODE>
__global__ __launch_bounds__(UE_THREADS) void k_unesc_write(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, const uint8_t* __restrict__ state,
                                                            const uint32_t* __restrict__ prefix, uint8_t* __restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[UE_WAVES][STAGE_BYTES / 4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t* const sd = stage[wv];
    uint8_t* const sb = reinterpret_cast<uint8_t*>(sd);
    for (uint32_t base = blockIdx.x * UE_WAVES; base < n_tiles; base += gridDim.x * UE_WAVES) {
        const uint32_t t = base + wv;
        const bool live = t < n_tiles;
        uint32_t P = 0, L = 0;
        if (live) {
            P = prefix[t];
            L = min(prefix[t + 1] - P, TILE_OUT_MAX);   // what the count pass found, built from the same decode()
            if (P > len || L > len - P) L = 0;          // the text is never longer than the input, and the buffer is sized by that
            Window w;
            uint4 raw;
            bool literal;
            if (lane_window<MODE>(data, len, t, lane, MODE == MODE_JSON ? state[t] : 0u, w, raw, literal)) {
                *reinterpret_cast<uint4*>(sd + lane * 4u) = raw;
            } else {
                uint32_t mine = lane_valid(len, t, lane);
                if (!literal) {
                    mine = 0;
#pragma unroll
                    for (uint32_t k = 0; k < LANE_BYTES; ++k) mine += item_len(w, OWN + k, MODE);
                }
                uint32_t pos = wave_exclusive(mine, lane);
                if (literal) {
#pragma unroll
                    for (uint32_t k = 0; k < LANE_BYTES; ++k, ++pos)
                        if (k < mine && pos < L) sb[pos] = (uint8_t)w.b[OWN + k];
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < LANE_BYTES; ++k) {
                        const Item it = decode(w, OWN + k, MODE);
                        uint32_t b = it.bytes;
                        for (uint32_t j = 0; j < it.len; ++j, ++pos, b >>= 8)
                            if (pos < L) sb[pos] = (uint8_t)b;
                    }
                }
            }
        }
        __syncthreads();
        if (live && L) {
            // the tile's output is text[P, P + L). With s = P % 16, byte q of it lies at 16-byte line (s + q) / 16 of the text counted from
            // P - s: lines c0 .. c1 - 1 are all this tile's
            const uint32_t s = P & 15u, e = s + L;
            const uint32_t c0 = (s + 15u) >> 4, c1 = e >> 4;
            const uint32_t head_end = min(c0 * 16u, e);                // head: [s, head_end)
            const uint32_t tail_begin = c1 >= c0 ? c1 * 16u : e;       // tail: [tail_begin, e)
            if (lane < head_end - s) text[(size_t)P + lane] = sb[lane];
            if (lane < e - tail_begin) { const uint32_t q = tail_begin - s + lane; text[(size_t)P + q] = sb[q]; }
            uint8_t* const lines = text + ((size_t)P - s);
            const uint32_t sh = ((16u - s) & 3u) * 8u;                  // (16 c - s) % 4 bytes, the same for every line
            for (uint32_t c = c0 + lane; c < c1; c += 64u) {
                const uint32_t q = c * 16u - s, dq = q >> 2;            // q + 16 <= L: the five dwords end at or in front of byte L + 4 of the stage
                uint32_t d[5];
#pragma unroll
                for (uint32_t k = 0; k < 5u; ++k) d[k] = sd[dq + k];
                uint4 o;
                o.x = (uint32_t)((((uint64_t)d[1] << 32) | d[0]) >> sh);
                o.y = (uint32_t)((((uint64_t)d[2] << 32) | d[1]) >> sh);
                o.z = (uint32_t)((((uint64_t)d[3] << 32) | d[2]) >> sh);
                o.w = (uint32_t)((((uint64_t)d[4] << 32) | d[3]) >> sh);
                *reinterpret_cast<uint4*>(lines + (size_t)c * 16u) = o;
            }
        }
        __syncthreads();
    }
}

// ---- the state of every tile (JSON) ---------------------------------------------------------------------------------------------------
// codes[t], t < n_codes: the tiles in front of the last one, all full
__global__ __launch_bounds__(UE_THREADS) void k_unesc_code(const uint8_t* __restrict__ data, uint32_t n_codes, uint32_t* __restrict__ codes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = (blockIdx.x * UE_THREADS + threadIdx.x) & ~63u, t = first + lane;
    const bool live = t < n_codes;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (live) v = *reinterpret_cast<const uint4*>(data + (size_t)t * TILE_BYTES + (TILE_BYTES - 16u));
    const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
    uint32_t tail[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) tail[k] = byte_of(vw[k >> 2], k & 3u);
    uint32_t from = 0, e0 = 0;
    bool fixed = false;   // a byte other than a backslash among the first ten: esc is 0 behind it
#pragma unroll
    for (uint32_t k = 0; k < 10u; ++k)
        if (tail[k] != '\\') { from = k + 1u; fixed = true; }
    // the tiles of this wave whose run may begin further in front, the whole wave on each: lane i reads bytes 16 i .. 16 i + 15 of the
    // tile (lane 63: the tail again, not used). Four tiles a round, so that their loads are in flight together.
    for (uint64_t todo = __ballot(live && !fixed); todo;) {
        uint32_t l[4];
        uint4 x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            l[j] = todo ? (uint32_t)__ffsll((unsigned long long)todo) - 1u : 64u;
            todo &= todo - 1ull;   // stays 0
            x[j] = make_uint4(0, 0, 0, 0);
            if (l[j] < 64u) x[j] = *reinterpret_cast<const uint4*>(data + (size_t)(first + l[j]) * TILE_BYTES + lane * 16u);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            if (l[j] == 64u) continue;
            const uint32_t xw[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
            uint32_t bs = 0;
#pragma unroll
            for (uint32_t k = 0; k < 16u; ++k) bs |= (uint32_t)(byte_of(xw[k >> 2], k & 3u) == '\\') << k;
            const uint32_t run = trailing_run(bs);
            const uint64_t broken = __ballot(lane < 63u && run != 16u);
            uint32_t e = 2u;   // backslashes from the tile's first byte on, an even number of them: esc of tail[0] is the tile's own state
            if (broken) {
                const uint32_t h = 63u - (uint32_t)__clzll((long long)broken);
                e = (__shfl(run, (int)h) & 1u) ? 3u : 0u;   // the lanes between h and the tail hold 16 each: the parity is lane h's
            }
            if (lane == l[j]) e0 = e;
        }
    }
    if (live) codes[t] = tail_code(tail, from, e0);
}

// inclusive ordered composition over the threads of a workgroup; s[i] holds thread i's result afterwards
__device__ __forceinline__ uint32_t block_compose(uint32_t f, uint32_t* s) {
    s[threadIdx.x] = f;
    __syncthreads();
    for (uint32_t off = 1; off < UE_THREADS; off <<= 1) {
        const uint32_t p = threadIdx.x >= off ? s[threadIdx.x - off] : FN_IDENTITY;
        __syncthreads();
        f = fn_compose(p, f);
        s[threadIdx.x] = f;
        __syncthreads();
    }
    return f;
}

__global__ __launch_bounds__(UE_THREADS) void k_unesc_chunk(const uint32_t* __restrict__ codes, uint32_t n_codes, uint32_t* __restrict__ fns) {
    __shared__ uint32_t s[UE_THREADS];
    const uint32_t t0 = blockIdx.x * UNESCAPE_STATE_CHUNK + threadIdx.x * STATE_ITEMS;
    uint32_t f = FN_IDENTITY;
#pragma unroll
    for (uint32_t r = 0; r < STATE_ITEMS; ++r)
        if (t0 + r < n_codes) f = fn_compose(f, fn_of(codes[t0 + r]));
    f = block_compose(f, s);
    if (threadIdx.x == UE_THREADS - 1) fns[blockIdx.x] = f;
}

// state[0] = 0, state[t + 1] = code_apply(codes[t], state[t]) for t < n_codes (thread i owns STATE_ITEMS consecutive tiles of the chunk)
__global__ __launch_bounds__(UE_THREADS) void k_unesc_scan(const uint32_t* __restrict__ codes, uint32_t n_codes, const uint32_t* __restrict__ fns,
                                                           uint8_t* __restrict__ state) {
    __shared__ uint32_t s[UE_THREADS];
    const uint32_t per = (blockIdx.x + UE_THREADS - 1) / UE_THREADS;   // chunks in front of this one, a slice per thread
    uint32_t f = FN_IDENTITY;
    for (uint32_t c = threadIdx.x * per; c < min((threadIdx.x + 1u) * per, blockIdx.x); ++c) f = fn_compose(f, fns[c]);
    (void)block_compose(f, s);
    const uint32_t before = s[UE_THREADS - 1];
    __syncthreads();
    const uint32_t t0 = blockIdx.x * UNESCAPE_STATE_CHUNK + threadIdx.x * STATE_ITEMS;
    uint32_t c[STATE_ITEMS];
    f = FN_IDENTITY;
#pragma unroll
    for (uint32_t r = 0; r < STATE_ITEMS; ++r) {
        c[r] = t0 + r < n_codes ? codes[t0 + r] : 0u;
        if (t0 + r < n_codes) f = fn_compose(f, fn_of(c[r]));
    }
    (void)block_compose(f, s);
    const uint32_t excl = threadIdx.x ? s[threadIdx.x - 1] : FN_IDENTITY;
    uint32_t st = fn_compose(before, excl) & 1u;   // the batch begins with esc = 0: bit 0 of the function is its value there
    if (t0 == 0) state[0] = 0;
#pragma unroll
    for (uint32_t r = 0; r < STATE_ITEMS; ++r) {
        if (t0 + r < n_codes) {
            st = code_apply(c[r], st);
            state[t0 + r + 1] = (uint8_t)st;
        }
    }
}

uint32_t grid_for_tiles(uint32_t n_tiles, int n_cu) {
    return std::min<uint32_t>((n_tiles + UE_WAVES - 1) / UE_WAVES, (uint32_t)std::max(n_cu, 1) * 8u);
}
bool mode_ok(uint32_t mode) { return mode == MODE_PERCENT || mode == MODE_JSON; }

}  // namespace

uint32_t unescape_state_chunks(uint32_t n_tiles) { return (n_tiles + UNESCAPE_STATE_CHUNK - 1) / UNESCAPE_STATE_CHUNK; }

hipError_t unescape_states(const uint8_t* data, uint32_t len, uint32_t* codes, uint32_t* fns, uint8_t* state, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)unescape::tiles(len);
    if (n_tiles == 0) return hipSuccess;
    if (len >= 0x7FFF0000u) return hipErrorInvalidValue;
    const uint32_t n_codes = n_tiles - 1, chunks = unescape_state_chunks(n_tiles);   // chunks >= 1: state[0] has a writer
    if (n_codes) {
        hipLaunchKernelGGL(k_unesc_code, dim3((n_codes + UE_THREADS - 1) / UE_THREADS), dim3(UE_THREADS), 0, stream, data, n_codes, codes);
        hipLaunchKernelGGL(k_unesc_chunk, dim3(chunks), dim3(UE_THREADS), 0, stream, (const uint32_t*)codes, n_codes, fns);
    }
    hipLaunchKernelGGL(k_unesc_scan, dim3(chunks), dim3(UE_THREADS), 0, stream, (const uint32_t*)codes, n_codes, (const uint32_t*)fns, state);
    return hipGetLastError();
}

hipError_t unescape_count(const uint8_t* data, uint32_t len, uint32_t mode, const uint8_t* state, uint32_t* counts, UnescapeCounters* ctr, int n_cu, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)unescape::tiles(len);
    if (n_tiles == 0) return hipSuccess;
    if (!mode_ok(mode) || len >= 0x7FFF0000u) return hipErrorInvalidValue;
    const uint32_t grid = grid_for_tiles(n_tiles, n_cu);
    if (mode == MODE_JSON) hipLaunchKernelGGL(k_unesc_count<MODE_JSON>, dim3(grid), dim3(UE_THREADS), 0, stream, data, len, n_tiles, state, counts, ctr);
    else hipLaunchKernelGGL(k_unesc_count<MODE_PERCENT>, dim3(grid), dim3(UE_THREADS), 0, stream, data, len, n_tiles, state, counts, ctr);
    return hipGetLastError();
}

hipError_t unescape_seal(const uint32_t* prefix, uint32_t n_tiles, UnescapeCounters* ctr, hipStream_t stream) {
    hipLaunchKernelGGL(k_unesc_seal, dim3(1), dim3(64), 0, stream, prefix, n_tiles, ctr);
    return hipGetLastError();
}

hipError_t unescape_write(const uint8_t* data, uint32_t len, uint32_t mode, const uint8_t* state, const uint32_t* prefix, uint8_t* text, int n_cu, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)unescape::tiles(len);
    if (n_tiles == 0) return hipSuccess;
    if (!mode_ok(mode) || len >= 0x7FFF0000u) return hipErrorInvalidValue;
    const uint32_t grid = grid_for_tiles(n_tiles, n_cu);
    if (mode == MODE_JSON) hipLaunchKernelGGL(k_unesc_write<MODE_JSON>, dim3(grid), dim3(UE_THREADS), 0, stream, data, len, n_tiles, state, prefix, text);
    else hipLaunchKernelGGL(k_unesc_write<MODE_PERCENT>, dim3(grid), dim3(UE_THREADS), 0, stream, data, len, n_tiles, state, prefix, text);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
namespace {
size_t grown(size_t n) { return n + n / 8 + 4096; }
}  // namespace

void Unescape::check(const uint8_t* src, size_t len, uint32_t modes) {
    if (modes == 0 || modes > (MODE_PERCENT | MODE_JSON)) throw ParamError{"unescape: modes is PERCENT (1), JSON (2) or both (3)"};
    if (!src && len) throw ParamError{"unescape: no input"};
    if (len >= 0x7FFF0000u) throw ParamError{"unescape: the input reaches 2^31 bytes; cut it into smaller batches"};
}

uint8_t* Unescape::input_buffer(size_t len) {
    if (in_.n < len) in_.alloc(grown(len));
    return in_.p;
}

// one run of the pass over `in` (device memory, 16-byte aligned, len > 0) into `text`; returns with text_len_ on the host
void Unescape::run(const uint8_t* in, uint32_t len, uint32_t mode, uint8_t* text, int n_cu, Event* ev, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)unescape::tiles(len);
    if (ev) MXY_HIP(hipEventRecord(ev[0], stream));
    if (mode == MODE_JSON) MXY_HIP(unescape_states(in, len, codes_.p, fns_.p, state_.p, stream));
    MXY_HIP(unescape_count(in, len, mode, state_.p, counts_.p, ctr_.p, n_cu, stream));
    if (ev) MXY_HIP(hipEventRecord(ev[1], stream));
    MXY_HIP(tile_prefix_build(counts_.p, n_tiles, chunks_.p, prefix_.p, stream));
    MXY_HIP(unescape_seal(prefix_.p, n_tiles, ctr_.p, stream));
    if (ev) MXY_HIP(hipEventRecord(ev[2], stream));
    // the scan's launch parameters are host values: the counter block comes back while the write step runs
    MXY_HIP(hipMemcpyAsync(host_.p, ctr_.p, 16, hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipEventRecord(ev_len_, stream));
    MXY_HIP(unescape_write(in, len, mode, state_.p, prefix_.p, text, n_cu, stream));
    if (ev) MXY_HIP(hipEventRecord(ev[3], stream));
    MXY_HIP(hipEventSynchronize(ev_len_));
    text_len_ = host_.p->text_len;
    if (text_len_ > len) throw HipError{"unescape: the prefix step reports more bytes than the input has"};
}

void Unescape::launch(const uint8_t* src, size_t len, uint32_t modes, int n_cu, bool profile, hipStream_t stream) {
    check(src, len, modes);
    if ((uintptr_t)src & 15u) throw ParamError{"unescape: the device input is not 16-byte aligned"};
    const uint32_t n_tiles = (uint32_t)unescape::tiles(len), chunks = line_chunks(n_tiles);
    const bool both = modes == (MODE_PERCENT | MODE_JSON);
    for (int k = 0; k < (both ? 2 : 1); ++k)
        if (text_[k].n < len + 16) text_[k].alloc(grown(len + 16));   // 16 spare bytes behind the batch, like every scanned buffer
    if (counts_.n < n_tiles || !prefix_.p) { counts_.alloc(grown(n_tiles)); prefix_.alloc(counts_.n + 1); }
    if (chunks_.n < chunks) chunks_.alloc((size_t)chunks + 64);
    if ((modes & MODE_JSON) && (codes_.n < n_tiles || !state_.p)) {
        codes_.alloc(grown(n_tiles)); state_.alloc(codes_.n); fns_.alloc(unescape_state_chunks((uint32_t)codes_.n) + 1);
    }
    if (!ctr_.p) ctr_.alloc(1);
    host_.ensure(1);
    ev_len_.create(hipEventDisableTiming);
    with_text_ = false;
    timed_ = false;
    *host_.p = UnescapeCounters{};
    text_len_ = 0;
    cur_ = 0;
    runs_ = 0;
    if (len == 0) return;
    timed_ = profile;
    if (profile) for (auto& row : ev_) for (Event& e : row) e.create();
    MXY_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(UnescapeCounters), stream));
    const uint8_t* in = src;
    uint32_t n = (uint32_t)len;
    for (const uint32_t mode : {MODE_JSON, MODE_PERCENT}) {   // JSON | PERCENT is percent(json(x))
        if (!(modes & mode) || n == 0) continue;
        const uint32_t dst = runs_;   // the first run writes text 0, the second reads it and writes text 1
        run(in, n, mode, text_[dst].p, n_cu, profile ? ev_[runs_] : nullptr, stream);
        in = text_[dst].p;
        n = text_len_;
        cur_ = dst;
        ++runs_;
    }
}

void Unescape::queue_results(bool with_text, hipStream_t stream) {
    with_text_ = with_text;
    if (!with_text || !text_len_) return;
    text_pinned_.ensure(text_len_, text_len_ / 8 + 4096);
    MXY_HIP(hipMemcpyAsync(text_pinned_.p, text_[cur_].p, text_len_, hipMemcpyDeviceToHost, stream));
}

Unescape::Result Unescape::finish() {
    Result r;
    r.text_len = text_len_;
    r.escapes = host_.p->escapes;
    r.replaced = host_.p->replaced;
    r.lf_escapes = host_.p->lf_escapes;
    if (with_text_) r.text = text_len_ ? text_pinned_.p : reinterpret_cast<const uint8_t*>("");
    if (timed_) {
        for (int k = 0; k < 3; ++k) ms_[k] = 0;
        for (uint32_t i = 0; i < runs_; ++i)
            for (int k = 0; k < 3; ++k) {
                float ms = 0;
                MXY_HIP(hipEventElapsedTime(&ms, ev_[i][k], ev_[i][k + 1]));
                ms_[k] += ms;
            }
    }
    return r;
}

}  // namespace mxy
