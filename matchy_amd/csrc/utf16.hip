// UTF-16 inputs, transcoded to UTF-8 on the GPU in front of the scan. The rules are utf16_core.h (unit_len / unit_bytes of an item and
// its two neighbours); this file is the three steps over tiles of TILE_BYTES input bytes, one wave per tile, lane l on bytes 16 l .. 16 l + 15
// (eight items):
//   k_utf16_count   output bytes of every tile. The neighbour across a lane boundary comes from a cross-lane move, the two neighbours
//                   across the tile's boundaries from one 2-byte load (lane 0 in front, lane 63 behind). The U+FFFD of the input are
//                   summed per wave and added to the counter block.
//   prefix          exclusive prefix over the tiles: the kernels of the line index (tile_prefix_build); k_utf16_seal puts the total and
//                   the number of code units into the counter block.
//   k_utf16_write   a wave stages its tile's output in LDS (at most TILE_OUT_MAX bytes) — each lane at the exclusive wave scan of its
//                   lengths — and stores the part of the tile's output range that covers whole 16-byte lines of the text as 16-byte
//                   stores; the ragged head and tail share lines with the neighbouring tiles and go out as byte stores. Every output
//                   byte is written by exactly one lane, and no kernel reads the text.
// A full tile whose units are all below 0x80 (an OR of its dwords against 0xFF80FF80) takes a fast path in both kernels: its length is
// TILE_UNITS, and its staged bytes are the packed low bytes. The store phase is shared, so the text is the same bytes either way.
// No load reaches data + len (the ragged end is read byte by byte), and nothing is stored without a bound that follows from the prefix.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "utf16.h"

namespace mxy {

namespace {

using namespace utf16;

constexpr uint32_t U16_THREADS = 256, U16_WAVES = U16_THREADS / 64;
// a 16-byte store is put together from five dwords of the stage: the last one may begin 12 bytes in front of the end of the output.
// A multiple of 16, so that every wave's stage is aligned for the 8-byte stores of the fast path.
constexpr uint32_t STAGE_BYTES = (TILE_OUT_MAX + 16 + 15) / 16 * 16;
static_assert(TILE_BYTES == 64 * 16, "a tile is one 16-byte load of every lane of a wave");

// 16 bytes at `off` (a multiple of 16; `data` is 16-byte aligned); bytes at or behind `len` read as zero and are not touched
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 16u <= len) return *reinterpret_cast<const uint4*>(data + off);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16u; ++k)
        if (off + k < len) w[k >> 2] |= (uint32_t)data[off + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t swap_units(uint32_t w) { return __byte_perm(w, 0u, 0x2301u); }   // both units of a dword: one permute

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

// The items of tile t (t * TILE_BYTES < len) as lane `lane` sees them: it[1..8] its own eight, it[0] the one in front, it[9] the one
// behind. `raw` is the lane's 16 bytes in unit order. Returns true, with `it` untouched, when the tile is full and all ASCII; the
// answer is the same in every lane. All 64 lanes call it.
template <bool BE>
__device__ __forceinline__ bool lane_items(const uint8_t* __restrict__ data, uint32_t len, uint32_t t, uint32_t lane, uint32_t (&it)[10], uint4& raw) {
    const uint32_t n_units = len >> 1, odd = len & 1u;
    const uint32_t off = t * TILE_BYTES + lane * 16u;   // below 2^31 + TILE_BYTES
    uint4 v = off < len ? load16(data, off, len) : make_uint4(0, 0, 0, 0);
    if (BE) { v.x = swap_units(v.x); v.y = swap_units(v.y); v.z = swap_units(v.z); v.w = swap_units(v.w); }
    raw = v;
    const uint32_t first = t * TILE_UNITS;
    if (first + TILE_UNITS <= n_units && __ballot(((v.x | v.y | v.z | v.w) & 0xFF80FF80u) != 0u) == 0ull) return true;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    const uint32_t u0 = first + lane * 8u;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint32_t unit = (w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu, idx = u0 + k;
        it[1 + k] = idx < n_units ? unit : (idx == n_units && odd) ? UNIT_ODD : UNIT_NONE;
    }
    uint32_t edge = UNIT_NONE;   // lane 0: the item in front of the tile; lane 63: the one behind it
    if ((lane == 0 && t != 0) || lane == 63) {
        const uint32_t idx = lane == 0 ? first - 1u : first + TILE_UNITS;
        if (idx < n_units) {
            const uint32_t h = *reinterpret_cast<const uint16_t*>(data + 2u * (size_t)idx);   // 2 idx + 1 < len
            edge = BE ? ((h >> 8) | ((h & 0xFFu) << 8)) : h;
        } else if (idx == n_units && odd) edge = UNIT_ODD;
    }
    const uint32_t p = __shfl_up(it[8], 1), n = __shfl_down(it[1], 1);
    it[0] = lane == 0 ? edge : p;
    it[9] = lane == 63 ? edge : n;
    return false;
}

template <bool BE>
__global__ __launch_bounds__(U16_THREADS) void k_utf16_count(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, uint32_t* __restrict__ counts,
                                                             Utf16Counters* __restrict__ ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * U16_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * U16_WAVES;
    uint32_t replaced = 0;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        uint32_t it[10];
        uint4 raw;
        uint32_t total = TILE_UNITS;
        if (!lane_items<BE>(data, len, t, lane, it, raw)) {
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                mine += unit_len(it[k], it[k + 1], it[k + 2]);
                replaced += it[k + 1] != UNIT_NONE && unit_replaced(it[k], it[k + 1], it[k + 2]);
            }
            total = wave_sum(mine);
        }
        if (lane == 0) counts[t] = total;
    }
    replaced = wave_sum(replaced);
    if (lane == 0 && replaced) atomicAdd(&ctr->replaced, replaced);
}

__global__ void k_utf16_seal(const uint32_t* __restrict__ prefix, uint32_t n_tiles, uint32_t len, Utf16Counters* __restrict__ ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { ctr->text_len = prefix[n_tiles]; ctr->code_units = len >> 1; }
}

__device__ __forceinline__ uint32_t low_bytes(uint32_t a, uint32_t b) {   // the low bytes of the four units of two dwords
    return (a & 0xFFu) | ((a >> 8) & 0xFF00u) | ((b & 0xFFu) << 16) | ((b << 8) & 0xFF000000u);
}

// The waves of a workgroup take the same number of rounds (a wave without a tile in the last round idles through it), so the barriers
// between the stage's writers and readers are met by all of them.
template <bool BE>
__global__ __launch_bounds__(U16_THREADS) void k_utf16_write(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, const uint32_t* __restrict__ prefix,
                                                             uint8_t* __restrict__ text) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[U16_WAVES][STAGE_BYTES / 4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t* const sd = stage[w];
    uint8_t* const sb = reinterpret_cast<uint8_t*>(sd);
    for (uint32_t base = blockIdx.x * U16_WAVES; base < n_tiles; base += gridDim.x * U16_WAVES) {
        const uint32_t t = base + w;
        const bool live = t < n_tiles;
        uint32_t P = 0, L = 0;
        if (live) {
            P = prefix[t];
            L = min(prefix[t + 1] - P, TILE_OUT_MAX);   // what the count pass found, built from the same unit_len
            uint32_t it[10];
            uint4 raw;
            if (lane_items<BE>(data, len, t, lane, it, raw)) {
                *reinterpret_cast<uint2*>(sd + lane * 2u) = make_uint2(low_bytes(raw.x, raw.y), low_bytes(raw.z, raw.w));
            } else {
                uint32_t mine = 0;
#pragma unroll
                for (uint32_t k = 0; k < 8u; ++k) mine += unit_len(it[k], it[k + 1], it[k + 2]);
                uint32_t pos = wave_exclusive(mine, lane);
#pragma unroll
                for (uint32_t k = 0; k < 8u; ++k) {
                    const uint32_t l = unit_len(it[k], it[k + 1], it[k + 2]);
                    uint32_t b = unit_bytes(it[k], it[k + 1], it[k + 2]);
                    for (uint32_t j = 0; j < l; ++j, ++pos, b >>= 8)
                        if (pos < L) sb[pos] = (uint8_t)b;
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

uint32_t grid_for_tiles(uint32_t n_tiles, int n_cu) {
    return std::min<uint32_t>((n_tiles + U16_WAVES - 1) / U16_WAVES, (uint32_t)std::max(n_cu, 1) * 8u);
}

}  // namespace

hipError_t utf16_count(const uint8_t* data, uint32_t len, uint32_t order, uint32_t* counts, Utf16Counters* ctr, int n_cu, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)utf16::tiles(len);
    if (n_tiles == 0) return hipSuccess;
    if (order > utf16::ORDER_BE || out_bound(len) >= (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t grid = grid_for_tiles(n_tiles, n_cu);
    if (order == utf16::ORDER_BE) hipLaunchKernelGGL(k_utf16_count<true>, dim3(grid), dim3(U16_THREADS), 0, stream, data, len, n_tiles, counts, ctr);
    else hipLaunchKernelGGL(k_utf16_count<false>, dim3(grid), dim3(U16_THREADS), 0, stream, data, len, n_tiles, counts, ctr);
    return hipGetLastError();
}

hipError_t utf16_seal(const uint32_t* prefix, uint32_t n_tiles, uint32_t len, Utf16Counters* ctr, hipStream_t stream) {
    hipLaunchKernelGGL(k_utf16_seal, dim3(1), dim3(64), 0, stream, prefix, n_tiles, len, ctr);
    return hipGetLastError();
}

hipError_t utf16_write(const uint8_t* data, uint32_t len, uint32_t order, const uint32_t* prefix, uint8_t* text, int n_cu, hipStream_t stream) {
    const uint32_t n_tiles = (uint32_t)utf16::tiles(len);
    if (n_tiles == 0) return hipSuccess;
    if (order > utf16::ORDER_BE || out_bound(len) >= (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t grid = grid_for_tiles(n_tiles, n_cu);
    if (order == utf16::ORDER_BE) hipLaunchKernelGGL(k_utf16_write<true>, dim3(grid), dim3(U16_THREADS), 0, stream, data, len, n_tiles, prefix, text);
    else hipLaunchKernelGGL(k_utf16_write<false>, dim3(grid), dim3(U16_THREADS), 0, stream, data, len, n_tiles, prefix, text);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
namespace {
size_t grown(size_t n) { return n + n / 8 + 4096; }
}  // namespace

void Utf16Transcode::check(const uint8_t* src, size_t len, uint32_t order) {
    if (order > utf16::ORDER_BE) throw ParamError{"utf16: byte_order is 0 (little-endian) or 1 (big-endian)"};
    if (!src && len) throw ParamError{"utf16: no input"};
    if (out_bound(len) >= (1ull << 31)) throw ParamError{"utf16: the input may transcode to 2^31 bytes or more (3 bytes per code unit); cut it into smaller batches"};
}

uint8_t* Utf16Transcode::input_buffer(size_t len) {
    if (in_.n < len) in_.alloc(grown(len));
    return in_.p;
}

void Utf16Transcode::launch(const uint8_t* src, size_t len, uint32_t order, int n_cu, bool profile, hipStream_t stream) {
    check(src, len, order);
    if ((uintptr_t)src & 15u) throw ParamError{"utf16: the device input is not 16-byte aligned"};
    const uint64_t bound = out_bound(len);
    const uint32_t n_tiles = (uint32_t)utf16::tiles(len), chunks = line_chunks(n_tiles);
    if (text_.n < bound + 16) text_.alloc(grown(bound + 16));   // 16 spare bytes behind the batch, like every scanned buffer
    if (counts_.n < n_tiles || !prefix_.p) { counts_.alloc(grown(n_tiles)); prefix_.alloc(counts_.n + 1); }
    if (chunks_.n < chunks) chunks_.alloc((size_t)chunks + 64);
    if (!ctr_.p) ctr_.alloc(1);
    host_.ensure(1);
    ev_len_.create(hipEventDisableTiming);
    with_text_ = false;
    timed_ = false;
    *host_.p = Utf16Counters{};
    text_len_ = 0;
    if (len == 0) return;
    const uint8_t* in = src;
    timed_ = profile;
    if (profile) {
        for (Event& e : ev_) e.create();
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    MXY_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(Utf16Counters), stream));
    MXY_HIP(utf16_count(in, (uint32_t)len, order, counts_.p, ctr_.p, n_cu, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[1], stream));
    MXY_HIP(tile_prefix_build(counts_.p, n_tiles, chunks_.p, prefix_.p, stream));
    MXY_HIP(utf16_seal(prefix_.p, n_tiles, (uint32_t)len, ctr_.p, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[2], stream));
    // the scan's launch parameters are host values: the counter block comes back while the write step runs
    MXY_HIP(hipMemcpyAsync(host_.p, ctr_.p, 16, hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipEventRecord(ev_len_, stream));
    MXY_HIP(utf16_write(in, (uint32_t)len, order, prefix_.p, text_.p, n_cu, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[3], stream));
    MXY_HIP(hipEventSynchronize(ev_len_));
    text_len_ = host_.p->text_len;
    if (text_len_ > bound) throw HipError{"utf16: the prefix step reports more bytes than the input can give"};
}

void Utf16Transcode::queue_results(bool with_text, hipStream_t stream) {
    with_text_ = with_text;
    if (!with_text || !text_len_) return;
    text_pinned_.ensure(text_len_, text_len_ / 8 + 4096);
    MXY_HIP(hipMemcpyAsync(text_pinned_.p, text_.p, text_len_, hipMemcpyDeviceToHost, stream));
}

Utf16Transcode::Result Utf16Transcode::finish() {
    Result r;
    r.text_len = text_len_;
    r.code_units = host_.p->code_units;
    r.replaced = host_.p->replaced;
    if (with_text_) r.text = text_len_ ? text_pinned_.p : reinterpret_cast<const uint8_t*>("");
    if (timed_) for (int k = 0; k < 3; ++k) MXY_HIP(hipEventElapsedTime(&ms_[k], ev_[k], ev_[k + 1]));
    return r;
}

}  // namespace mxy
