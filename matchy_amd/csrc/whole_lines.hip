// Whole-line queries on the GPU: every line of the batch is one query (`matchy match --whole-lines`, matchy_scanner_set_whole_lines).
// The front end replaces k_anchor and the validators; behind it the lookup passes run unchanged over the candidate list it writes.
//   line_index_build   '\n' counts per WL_TILE-byte tile and their exclusive prefix (line_index.hip)
//   k_wl_scatter       second streaming pass: lane l of a wave holds bytes 16 l .. 16 l + 15 of a tile; a '\n' at position p whose rank
//                      in the batch is r (prefix of the tile + '\n' bytes of the lanes in front + those in front of it in the lane)
//                      writes ends[r] = p. Line r is [ends[r - 1] + 1, ends[r]): no lane ever searches for an end of its line. The same
//                      lane judges the bytes >= 0x80 among its 16 by wl::utf8_byte_bad, from at most three bytes on either side (the
//                      neighbouring lanes' registers), and marks the line of a bad byte.
//   k_wl_classify      one lane per line: strips the '\r', runs parse_ip over a query of at most 45 bytes and writes candidate r.
//                      IPv6 queries are answered here (trie_v6 + pack_record): k_lookup re-parses IPv6 text with a parser that knows
//                      no embedded dotted quad.
// A lane reads at most 22 bytes per tile step and at most 46 bytes of a query: 5 MB in one line or in 5 M empty lines cost what 5 MB
// of ordinary lines cost. Query k is candidate k whatever order the waves run in; past the capacity of the arrays the kernels count
// and do not write (Scanner::fetch regrows and scans again).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_shared.h"
#include "whole_lines.h"
#include "whole_lines_core.h"

namespace mxy {

namespace {

constexpr uint32_t WL_THREADS = 256, WL_WAVES = WL_THREADS / 64;
constexpr uint32_t WL_WG_TILES = WL_WG_CHUNK / WL_TILE, WL_WAVE_TILES = WL_WG_TILES / WL_WAVES;

// `n` bytes (a multiple of 4, at most 16) at `off` (a multiple of 4; `data` is 16-byte aligned); bytes at or behind `len` read as zero and are not touched
__device__ __forceinline__ uint32_t load4(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 4u <= len) return *reinterpret_cast<const uint32_t*>(data + off);
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4u; ++k)
        if (off + k < len) w |= (uint32_t)data[off + k] << (8 * k);
    return w;
}
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 16u <= len) return *reinterpret_cast<const uint4*>(data + off);
    return make_uint4(load4(data, off, len), load4(data, off + 4u, len), load4(data, off + 8u, len), load4(data, off + 12u, len));
}
// bit k = byte k of the 16 is '\n'
__device__ __forceinline__ uint32_t nl_mask16(uint4 v) {
    auto pack = [](uint32_t z) { return (((z >> 7) * 0x00204081u) >> 21) & 0xFu; };   // bits 7, 15, 23, 31 -> bits 0..3
    return pack(nl_bytes(v.x)) | (pack(nl_bytes(v.y)) << 4) | (pack(nl_bytes(v.z)) << 8) | (pack(nl_bytes(v.w)) << 12);
}

__global__ __launch_bounds__(WL_THREADS) void k_wl_scatter(WholeLineParams p, uint32_t n_tiles) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_chunks = (n_tiles + WL_WG_TILES - 1) / WL_WG_TILES;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        for (uint32_t j = 0; j < WL_WAVE_TILES; ++j) {
            const uint32_t tile = chunk * WL_WG_TILES + wave * WL_WAVE_TILES + j;   // wave-uniform
            if (tile >= n_tiles) break;
            const uint32_t off = tile * WL_TILE + lane * WL_LANE_BYTES;            // < 2^31 + WL_TILE
            const bool have = off < p.len;
            const uint4 v = have ? load16(p.data, off, p.len) : make_uint4(0, 0, 0, 0);
            const uint32_t m = nl_mask16(v), c = __popc(m);
            uint32_t incl = c;   // '\n' bytes of this lane and the lanes in front of it
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, d);
                if (lane >= d) incl += t;
            }
            const uint32_t rank0 = p.prefix[tile] + incl - c;   // lines in front of the lane's first byte
            uint32_t r = rank0;
            for (uint32_t mm = m; mm; mm &= mm - 1u, ++r)
                if (r < p.cap) p.ends[r] = off + (uint32_t)__ffs(mm) - 1u;
            // UTF-8: the lane's 16 bytes between the last 4 of the lane in front and the first 4 of the lane behind
            uint32_t prev = (uint32_t)__shfl_up((int)v.w, 1), next = (uint32_t)__shfl_down((int)v.x, 1);
            if (((v.x | v.y | v.z | v.w) & 0x80808080u) == 0u || !have) continue;   // ASCII bytes are valid wherever they stand
            if (lane == 0) prev = off ? *reinterpret_cast<const uint32_t*>(p.data + off - 4u) : 0u;   // off <= len - 1: the four bytes exist
            if (lane == 63) next = off + 16u < p.len ? load4(p.data, off + 16u, p.len) : 0u;
            const uint32_t w[6] = {prev, v.x, v.y, v.z, v.w, next};
            auto byte_at = [&](int k) -> uint32_t { return (w[(k + 4) >> 2] >> (8 * ((k + 4) & 3))) & 0xFFu; };   // k = -4 .. 19
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t i = off + (uint32_t)k;
                const uint32_t b0 = byte_at(k);
                if (b0 < 0x80u || i >= p.len) continue;
                const uint32_t back = i < 3u ? i : 3u, ahead = p.len - 1u - i < 3u ? p.len - 1u - i : 3u;
                if (!wl::utf8_byte_bad(byte_at(k - 3), byte_at(k - 2), byte_at(k - 1), b0, byte_at(k + 1), byte_at(k + 2), byte_at(k + 3), back, ahead)) continue;
                const uint32_t line = rank0 + __popc(m & ((1u << k) - 1u));
                if (line < p.cap) p.invalid[line] = 1;   // every writer stores the same value
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
    return v;   // lane 0
}

// The parser walks a text byte by byte and every step depends on the byte before it: over global memory that is a chain of a dozen
// round trips per line. A lane therefore fetches the at most 45 bytes of a query that can be an address with independent 4-byte
// loads into a row of LDS of its own and parses there (scatter + classify over 10 M lines: 0.58 -> 0.48 ms; the kernel is still what
// the front end costs — 0.06 ms of it are the scatter pass — and its gathers of unaligned words are the suspect).
constexpr uint32_t WL_ROW_WORDS = 13;   // 48 bytes of text + one word: an odd stride keeps the lanes' rows on different banks
static_assert(WL_ROW_WORDS * 4 >= wl::ADDR_TEXT_MAX + 3, "a row holds the longest text the parser reads, in whole words");

__global__ __launch_bounds__(WL_THREADS) void k_wl_classify(WholeLineParams p, DevDb db, uint32_t n_tiles) {
    __shared__ uint32_t rows[WL_THREADS * WL_ROW_WORDS];
    uint32_t* row = rows + threadIdx.x * WL_ROW_WORDS;
    const uint32_t newlines = p.prefix[n_tiles];
    const uint32_t lines = wl::line_count(p.len, newlines, p.len ? p.data[p.len - 1u] : (uint8_t)0);
    const uint32_t n = min(lines, p.cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.counters->n_cand = lines;   // the demand: Scanner::fetch regrows the arrays when it exceeds their capacity
        p.counters->lines = newlines;
        p.wl->queries = lines;
    }
    uint32_t n_addr = 0, n_str = 0, n_bad = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += stride) {   // wave-uniform bound: pack_record is a wave operation
        const uint32_t r = base + threadIdx.x;
        Candidate c{0, 0xFFFFFFFFu, 0, 0};
        Hit h{};
        bool emit = false;
        if (r < n) {
            const uint32_t s = wl::line_start(p.ends, r);
            const uint32_t e = wl::query_end(p.data, s, wl::line_end(p.ends, newlines, p.len, r));
            const uint32_t ql = e - s;
            if (p.invalid[r]) ++n_bad;
            else if (ql >= wl::QUERY_LEN_LIMIT) atomicOr(&p.counters->error, 4u);
            else {
                IpAddr a;
                wl::QueryClass qc = wl::Q_STRING;
                if (ql < wl::ADDR_TEXT_MAX) {
#pragma unroll
                    for (uint32_t k = 0; k < (wl::ADDR_TEXT_MAX + 2) / 4; ++k) {
                        const uint32_t at = s + 4u * k;
                        uint32_t w = 0;
                        if (4u * k < ql) {
                            if (at + 4u <= p.len) __builtin_memcpy(&w, p.data + at, 4);   // may reach past the query, never past the batch
                            else for (uint32_t b = 0; at + b < p.len; ++b) w |= (uint32_t)p.data[at + b] << (8 * b);
                        }
                        row[k] = w;
                    }
                    qc = wl::classify(reinterpret_cast<const uint8_t*>(row), ql, a);
                }
                if (qc == wl::Q_STRING) { c = Candidate{s, ql | ((uint32_t)IT_DOMAIN << 24), 0, 0}; ++n_str; }
                else if (qc == wl::Q_IPV4) {
                    c = Candidate{s, ql | ((uint32_t)IT_IPV4 << 24), ((uint32_t)a.b[0] << 24) | ((uint32_t)a.b[1] << 16) | ((uint32_t)a.b[2] << 8) | a.b[3], 0};
                    ++n_addr;
                } else {
                    ++n_addr;
                    uint16_t seg[8];
                    for (int k = 0; k < 8; ++k) seg[k] = (uint16_t)(((uint32_t)a.b[2 * k] << 8) | a.b[2 * k + 1]);
                    uint32_t off, pfx;
                    if (db.has_ip && trie_v6(db, seg, off, pfx)) {
                        h.cand = r; h.start = s; h.len_type = ql | ((uint32_t)IT_IPV6 << 24);
                        h.kind = 2; h.a = off; h.prefix_len = (uint8_t)pfx;
                        emit = true;
                    }
                }
            }
            p.cands[r] = c;
        }
        pack_record(p.pk, emit, h, nullptr);
    }
    // the workgroup's sums leave with one atomic (two when it met invalid lines); ScanCounters::cand_true is their sum, taken by the host
    __shared__ uint32_t sums[WL_WAVES][3];
    const uint32_t ta = wave_sum(n_addr), ts = wave_sum(n_str), tb = wave_sum(n_bad);
    if ((threadIdx.x & 63u) == 0) { sums[threadIdx.x >> 6][0] = ta; sums[threadIdx.x >> 6][1] = ts; sums[threadIdx.x >> 6][2] = tb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, s = 0, b = 0;
        for (uint32_t w = 0; w < WL_WAVES; ++w) { a += sums[w][0]; s += sums[w][1]; b += sums[w][2]; }
        if (a | s) atomicAdd(&p.wl->address_string, (unsigned long long)a | ((unsigned long long)s << 32));
        if (b) atomicAdd(&p.wl->invalid_utf8, b);
    }
}

}  // namespace

void launch_whole_lines_scatter(const WholeLineParams& p, int n_cu, hipStream_t stream) {
    const uint32_t n_tiles = line_tiles(p.len);
    if (n_tiles == 0) return;
    const uint32_t n_chunks = (n_tiles + WL_WG_TILES - 1) / WL_WG_TILES;
    const uint32_t grid = std::min<uint32_t>(n_chunks, (uint32_t)std::max(n_cu, 1) * 8u);
    hipLaunchKernelGGL(k_wl_scatter, dim3(grid), dim3(WL_THREADS), 0, stream, p, n_tiles);
    check_launch("launch_whole_lines_scatter");
}

void launch_whole_lines_classify(const WholeLineParams& p, const DevDb& db, int n_cu, hipStream_t stream) {
    // one lane per line of the capacity at most; a batch of fewer lines leaves the workgroups behind them at once
    const uint32_t want = (p.cap + WL_THREADS - 1) / WL_THREADS;
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(want, (uint32_t)std::max(n_cu, 1) * 8u));
    hipLaunchKernelGGL(k_wl_classify, dim3(grid), dim3(WL_THREADS), 0, stream, p, db, line_tiles(p.len));
    check_launch("launch_whole_lines_classify");
}

}  // namespace mxy
