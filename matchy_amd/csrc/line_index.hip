// Line context of the hit records, on the GPU: for every hit the index of its line (number of '\n' in front of it) and where that
// line starts and ends, and per scan the number of distinct lines that carry a hit. The batch is resident in device memory when
// the scan ends; this is one more streaming pass over it, a prefix sum, and a short walk per hit:
//   k_line_count       '\n' bytes of every LINE_TILE-byte tile (16-byte coalesced loads, SWAR zero-byte test + popcount)
//   k_line_chunk_sum   counts of LINE_SCAN_CHUNK tiles -> one sum per chunk
//   k_line_scan        exclusive prefix over the tiles (one workgroup per chunk: the sums of the chunks in front of it, then a running
//                      sum over its own tiles; the shape of k_sort_scan with the repeated read cut down to the chunk sums), n_tiles + 1
//                      entries: the last one is the total
//   k_line_resolve     one lane per record: line = prefix of the tile + '\n' count of the tile's bytes in front of the hit; the line's
//                      ends from a byte search in the hit's own tile and, where that tile has no '\n' on that side, in the nearest
//                      tile that has one — found from the prefix array (neighbour first, then a binary search), never by reading the
//                      log: a single line of 40 MB costs a lane ~20 loads of prefixes and two tiles of bytes. The same lane inserts
//                      its line number into an open-addressing set; the inserts that claimed an empty slot are the distinct lines.
// Nothing here writes without a bound test, and no load of log bytes reaches `len` or beyond (the ragged end is read byte by byte).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "line_index.h"

namespace mxy {

namespace {

constexpr uint32_t LINE_THREADS = 256, LINE_WAVES = LINE_THREADS / 64;
constexpr uint32_t COUNT_UNROLL = 4;                       // tiles a wave has in flight
constexpr uint32_t SCAN_ITEMS = LINE_SCAN_CHUNK / LINE_THREADS;
static_assert(LINE_TILE == 64 * 16, "a tile is one 16-byte load of every lane of a wave");
static_assert(LINE_SCAN_CHUNK % LINE_THREADS == 0, "whole tiles per thread");

// 16 bytes at `off` (a multiple of 16; `data` is 16-byte aligned); bytes at or behind `len` read as zero and are not touched
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 16u <= len) return *reinterpret_cast<const uint4*>(data + off);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16u; ++k)
        if (off + k < len) w[k >> 2] |= (uint32_t)data[off + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint32_t nl_count16(uint4 v) {
    return __popc(nl_bytes(v.x)) + __popc(nl_bytes(v.y)) + __popc(nl_bytes(v.z)) + __popc(nl_bytes(v.w));
}
// bit k = byte k of the 16 is '\n'
__device__ __forceinline__ uint32_t nl_mask16(uint4 v) {
    auto pack = [](uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; };   // bits 7, 15, 23, 31 -> bits 0..3
    return pack(nl_bytes(v.x)) | (pack(nl_bytes(v.y)) << 4) | (pack(nl_bytes(v.z)) << 8) | (pack(nl_bytes(v.w)) << 12);
}

// Wave w takes COUNT_UNROLL consecutive tiles per round: lane l loads bytes 16 l .. 16 l + 15 of each, and the lanes' counts (0..16:
// five bits) are summed with one ballot per bit on the scalar side.
__global__ __launch_bounds__(LINE_THREADS) void k_line_count(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * LINE_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * LINE_WAVES;
    for (uint32_t t0 = wave * COUNT_UNROLL; t0 < n_tiles; t0 += n_waves * COUNT_UNROLL) {
        uint4 v[COUNT_UNROLL];
#pragma unroll
        for (uint32_t j = 0; j < COUNT_UNROLL; ++j) {
            const uint32_t off = (t0 + j) * LINE_TILE + lane * 16u;   // < 2^31 + COUNT_UNROLL * LINE_TILE
            v[j] = off < len ? load16(data, off, len) : make_uint4(0, 0, 0, 0);
        }
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t j = 0; j < COUNT_UNROLL; ++j) {
            const uint32_t c = nl_count16(v[j]);
            uint32_t total = 0;
#pragma unroll
            for (uint32_t b = 0; b < 5; ++b) total += (uint32_t)__popcll(__ballot((c >> b) & 1u)) << b;
            if (lane == j) mine = total;
        }
        if (lane < COUNT_UNROLL && t0 + lane < n_tiles) counts[t0 + lane] = mine;
    }
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s) {
    for (uint32_t off = 32; off; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < LINE_WAVES; ++w) t += s[w];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(LINE_THREADS) void k_line_chunk_sum(const uint32_t* __restrict__ counts, uint32_t n_tiles, uint32_t* __restrict__ chunk_sums) {
    __shared__ uint32_t s[LINE_WAVES];
    const uint32_t first = blockIdx.x * LINE_SCAN_CHUNK;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < SCAN_ITEMS; ++r) {
        const uint32_t t = first + r * LINE_THREADS + threadIdx.x;
        if (t < n_tiles) v += counts[t];
    }
    v = block_sum(v, s);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = v;
}

// prefix[t] = '\n' bytes in front of tile t, t = 0 .. n_tiles (thread i owns SCAN_ITEMS consecutive tiles of the chunk)
__global__ __launch_bounds__(LINE_THREADS) void k_line_scan(const uint32_t* __restrict__ counts, uint32_t n_tiles, const uint32_t* __restrict__ chunk_sums,
                                                            uint32_t* __restrict__ prefix) {
    __shared__ uint32_t s[LINE_THREADS];
    __shared__ uint32_t sw[LINE_WAVES];
    uint32_t before = 0;
    for (uint32_t c = threadIdx.x; c < blockIdx.x; c += LINE_THREADS) before += chunk_sums[c];
    before = block_sum(before, sw);
    const uint32_t t0 = blockIdx.x * LINE_SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
    uint32_t c[SCAN_ITEMS], own = 0;
#pragma unroll
    for (uint32_t r = 0; r < SCAN_ITEMS; ++r) { c[r] = t0 + r < n_tiles ? counts[t0 + r] : 0u; own += c[r]; }
    s[threadIdx.x] = own;
    __syncthreads();
    uint32_t incl = own;   // inclusive prefix over the threads' sums
    for (uint32_t off = 1; off < LINE_THREADS; off <<= 1) {
        const uint32_t t = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
        __syncthreads();
        incl += t;
        s[threadIdx.x] = incl;
        __syncthreads();
    }
    uint32_t run = before + incl - own;
#pragma unroll
    for (uint32_t r = 0; r < SCAN_ITEMS; ++r) {
        if (t0 + r < n_tiles) prefix[t0 + r] = run;
        run += c[r];
        if (t0 + r + 1 == n_tiles) prefix[n_tiles] = run;   // the total
    }
}

// One lane per record. STRIDE: bytes of a record (16: FinalHit, 8: compact IPv4 record); both begin with the start offset.
// set: open-addressing table of line numbers (LINE_SET_EMPTY = free), set_mask + 1 slots, a power of two of at least twice the records
// of the scan; nullptr = no distinct count. n_distinct: inserts that claimed a free slot, one atomic per wave.
template <uint32_t STRIDE>
__global__ __launch_bounds__(LINE_THREADS) void k_line_resolve(const uint8_t* __restrict__ data, uint32_t len, uint32_t n_tiles, const uint32_t* __restrict__ prefix,
                                                               const uint8_t* __restrict__ recs, uint32_t n, uint4* __restrict__ out,
                                                               uint32_t* __restrict__ set, uint32_t set_mask, uint32_t* __restrict__ n_distinct) {
    const uint32_t i = blockIdx.x * LINE_THREADS + threadIdx.x;
    const bool valid = i < n;
    bool claimed = false;
    if (valid) {
        const uint32_t s = min(*reinterpret_cast<const uint32_t*>(recs + (size_t)i * STRIDE), len);   // a record never starts behind the batch
        const uint32_t tile = s / LINE_TILE, base = tile * LINE_TILE, r = s - base;                   // tile <= n_tiles
        // the tile's bytes in front of s: their '\n' count, and the last of them
        uint32_t cnt = 0, start = 0;
        bool have_start = false;
        for (uint32_t w = 0; w * 16u < r; ++w) {
            uint32_t m = nl_mask16(load16(data, base + w * 16u, len));
            if (r - w * 16u < 16u) m &= (1u << (r - w * 16u)) - 1u;
            cnt += __popc(m);
            if (m) { start = base + w * 16u + (32u - __clz(m)); have_start = true; }
        }
        const uint32_t before = prefix[tile];
        const uint32_t line = before + cnt;
        if (!have_start && before) {
            // the nearest tile in front that has a '\n': the largest t with prefix[t] < before (prefix[0] = 0 < before)
            uint32_t t = tile - 1;
            if (prefix[t] >= before) {
                uint32_t lo = 0, hi = t;
                while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (prefix[mid] < before) lo = mid; else hi = mid; }
                t = lo;
            }
            for (uint32_t w = LINE_TILE / 16u; w-- > 0;) {
                const uint32_t m = nl_mask16(load16(data, t * LINE_TILE + w * 16u, len));
                if (m) { start = t * LINE_TILE + w * 16u + (32u - __clz(m)); break; }
            }
        }
        // the first '\n' at or behind s: in this tile, else in the nearest tile behind it that has one, else the line runs to the end
        uint32_t end = len;
        bool have_end = false;
        for (uint32_t w = r / 16u; w < LINE_TILE / 16u && base + w * 16u < len; ++w) {
            uint32_t m = nl_mask16(load16(data, base + w * 16u, len));
            if (w == r / 16u) m &= ~((1u << (r & 15u)) - 1u);
            if (m) { end = base + w * 16u + (uint32_t)__ffs(m) - 1u; have_end = true; break; }
        }
        if (!have_end && tile + 1 < n_tiles) {
            const uint32_t upto = prefix[tile + 1];
            if (prefix[n_tiles] > upto) {
                // the smallest t > tile with prefix[t + 1] > upto (t = n_tiles - 1 qualifies)
                uint32_t t = tile + 1;
                if (prefix[t + 1] <= upto) {
                    uint32_t lo = t, hi = n_tiles - 1;
                    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (prefix[mid + 1] > upto) hi = mid; else lo = mid; }
                    t = hi;
                }
                for (uint32_t w = 0; w < LINE_TILE / 16u && t * LINE_TILE + w * 16u < len; ++w) {
                    const uint32_t m = nl_mask16(load16(data, t * LINE_TILE + w * 16u, len));
                    if (m) { end = t * LINE_TILE + w * 16u + (uint32_t)__ffs(m) - 1u; break; }
                }
            }
        }
        out[i] = make_uint4(line, start, end, 0u);
        if (set) {
            uint32_t h = (line * 2654435761u) >> 7;
            for (uint32_t probe = 0; probe <= set_mask; ++probe, ++h) {
                const uint32_t old = atomicCAS(&set[h & set_mask], LINE_SET_EMPTY, line);
                if (old == LINE_SET_EMPTY) { claimed = true; break; }
                if (old == line) break;
            }
        }
    }
    if (set) {
        const uint64_t m = __ballot(claimed);
        if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((unsigned long long)m) - 1u) atomicAdd(n_distinct, (uint32_t)__popcll(m));
    }
}

}  // namespace

uint32_t line_tiles(uint32_t len) { return (uint32_t)(((uint64_t)len + LINE_TILE - 1) / LINE_TILE); }
uint32_t line_chunks(uint32_t n_tiles) { return (n_tiles + LINE_SCAN_CHUNK - 1) / LINE_SCAN_CHUNK; }

// counts: n_tiles entries; chunk_sums: line_chunks(n_tiles); prefix: n_tiles + 1
hipError_t line_index_build(const uint8_t* data, uint32_t len, uint32_t* counts, uint32_t* chunk_sums, uint32_t* prefix, int n_cu, hipStream_t stream,
                            hipEvent_t after_count) {
    const uint32_t n_tiles = line_tiles(len);
    if (n_tiles == 0) return hipMemsetAsync(prefix, 0, 4, stream);   // prefix[0] = 0: the total of an empty batch
    const uint32_t per_block = LINE_WAVES * COUNT_UNROLL;
    const uint32_t grid = std::min<uint32_t>((n_tiles + per_block - 1) / per_block, (uint32_t)std::max(n_cu, 1) * 8u);
    hipLaunchKernelGGL(k_line_count, dim3(grid), dim3(LINE_THREADS), 0, stream, data, len, n_tiles, counts);
    if (after_count) { const hipError_t e = hipEventRecord(after_count, stream); if (e != hipSuccess) return e; }
    return tile_prefix_build(counts, n_tiles, chunk_sums, prefix, stream);
}

// the prefix step alone, over any per-tile figures whose total stays below 2^32 (n_tiles > 0)
hipError_t tile_prefix_build(const uint32_t* counts, uint32_t n_tiles, uint32_t* chunk_sums, uint32_t* prefix, hipStream_t stream) {
    const uint32_t chunks = line_chunks(n_tiles);
    hipLaunchKernelGGL(k_line_chunk_sum, dim3(chunks), dim3(LINE_THREADS), 0, stream, counts, n_tiles, chunk_sums);
    hipLaunchKernelGGL(k_line_scan, dim3(chunks), dim3(LINE_THREADS), 0, stream, counts, n_tiles, (const uint32_t*)chunk_sums, prefix);
    return hipGetLastError();
}

hipError_t line_index_resolve(const uint8_t* data, uint32_t len, const uint32_t* prefix, const void* recs, uint32_t stride, uint32_t n, LineRec* out,
                              uint32_t* set, uint32_t set_slots, uint32_t* n_distinct, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (stride != 16 && stride != 8) return hipErrorInvalidValue;
    if (set && (set_slots < 2 || (set_slots & (set_slots - 1)) != 0)) return hipErrorInvalidValue;
    const uint32_t n_tiles = line_tiles(len), grid = (n + LINE_THREADS - 1) / LINE_THREADS;
    if (stride == 16)
        hipLaunchKernelGGL(k_line_resolve<16>, dim3(grid), dim3(LINE_THREADS), 0, stream, data, len, n_tiles, prefix, (const uint8_t*)recs, n,
                           reinterpret_cast<uint4*>(out), set, set_slots - 1, n_distinct);
    else
        hipLaunchKernelGGL(k_line_resolve<8>, dim3(grid), dim3(LINE_THREADS), 0, stream, data, len, n_tiles, prefix, (const uint8_t*)recs, n,
                           reinterpret_cast<uint4*>(out), set, set_slots - 1, n_distinct);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
void LineContext::resolve(const HitBatch& b, bool to_host, int n_cu, bool profile, hipStream_t stream) {
    auto grown = [](uint32_t n) { return (size_t)n + n / 4 + 1024; };
    const size_t n = (size_t)b.n_fin + b.n_c4;
    const uint32_t tiles = line_tiles(b.len), chunks = line_chunks(tiles);
    if (counts_.n < tiles || !prefix_.p) { counts_.alloc(grown(tiles)); prefix_.alloc(counts_.n + 1); }
    if (chunks_.n < chunks) chunks_.alloc((size_t)chunks + 64);
    if (!ctr_.p) ctr_.alloc(1);
    if (recs_.n < b.n_fin) recs_.alloc(grown(b.n_fin));
    if (c4_.n < b.n_c4) c4_.alloc(grown(b.n_c4));
    size_t slots = 1024;
    while (slots < 2 * n) slots <<= 1;
    if (set_.n < slots) set_.alloc(slots);
    set_slots_ = n ? (uint32_t)slots : 0u;
    const size_t head = sizeof(LineCounters), want = head + (to_host ? n * sizeof(LineRec) : 0);
    pinned_.ensure(want, want / 4 + (1 << 16));
    timed_ = profile;
    if (profile) {
        for (Event& e : ev_) e.create();
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    MXY_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(LineCounters), stream));
    if (n) MXY_HIP(hipMemsetAsync(set_.p, 0xFF, slots * 4, stream));
    MXY_HIP(line_index_build(b.data, b.len, counts_.p, chunks_.p, prefix_.p, n_cu, stream, profile ? (hipEvent_t)ev_[1] : nullptr));
    if (profile) { if (!tiles) MXY_HIP(hipEventRecord(ev_[1], stream)); MXY_HIP(hipEventRecord(ev_[2], stream)); }
    MXY_HIP(line_index_resolve(b.data, b.len, prefix_.p, b.fin, 16, b.n_fin, recs_.p, set_.p, (uint32_t)slots, &ctr_.p->distinct, stream));
    MXY_HIP(line_index_resolve(b.data, b.len, prefix_.p, b.c4, 8, b.n_c4, c4_.p, set_.p, (uint32_t)slots, &ctr_.p->distinct, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[3], stream));
    uint8_t* pb = pinned_.p;
    MXY_HIP(hipMemcpyAsync(pb, ctr_.p, sizeof(LineCounters), hipMemcpyDeviceToHost, stream));
    pending_ = Result{};
    if (to_host) {
        if (b.n_fin) MXY_HIP(hipMemcpyAsync(pb + head, recs_.p, (size_t)b.n_fin * sizeof(LineRec), hipMemcpyDeviceToHost, stream));
        if (b.n_c4) MXY_HIP(hipMemcpyAsync(pb + head + (size_t)b.n_fin * sizeof(LineRec), c4_.p, (size_t)b.n_c4 * sizeof(LineRec), hipMemcpyDeviceToHost, stream));
        pending_.fin_lines = b.n_fin ? (const LineRec*)(pb + head) : nullptr;
        pending_.c4_lines = b.n_c4 ? (const LineRec*)(pb + head) + b.n_fin : nullptr;
    }
}

LineContext::Result LineContext::finish() {
    pending_.lines_with_matches = reinterpret_cast<const LineCounters*>(pinned_.p)->distinct;
    if (timed_) for (int k = 0; k < 3; ++k) MXY_HIP(hipEventElapsedTime(&ms_[k], ev_[k], ev_[k + 1]));
    return pending_;
}

}  // namespace mxy
