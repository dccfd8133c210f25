// Extracted candidates as text, on the GPU: the candidates of an extraction scan in the order of `matchy extract` — by line, then by the
// line order of the item types, then by start — written as the command's json / csv / text output into one block in device memory.
// What the order and a byte of the text are decides extract_render_core.h; this file decides who computes them.
//   (line_index_build)  '\n' counts per 1 KiB tile and their exclusive prefix (line_index.hip)
//   k_xr_keys           one lane per list entry, XR_KEY_TILE entries per workgroup: the line of a real entry from the prefix of its
//                       tile and the '\n' bytes of the tile in front of it, the packed key, and the (key, list index) pairs of the
//                       workgroup compacted behind ONE add to the pair counter; the records per type through the LDS aggregator
//   (sort_pairs)        the pairs by key (the digit passes of sort_hits.hip)
//   k_xr_measure        one lane per sorted record: a candidate of at most XR_SHORT_MAX bytes is measured here (its escapes counted
//                       four bytes at a time), a longer one goes onto the long list
//   k_xr_long_measure   one wave per long record, 64 bytes per step
//   k_xr_chunk_sum      } exclusive prefix of the record lengths in 64 bits (the shape of k_rd_chunk_sum / k_rd_scan): rec_off, and
//   k_xr_scan           } the demand of the block
//   k_xr_write_short    a wave stages the text of its 64 records in LDS, window by window, and stores it with aligned 16-byte stores
//   k_xr_write_long     one wave per long record, 64 source bytes per step
// Every store to the block sits behind min(demand, capacity), the pair arrays and the long list behind n_real. Candidates are clamped
// to the batch before they are read: no load reaches data + len. Every loop names its bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "extract_render.h"
#include "extract_render_core.h"
#include "lds_aggregator.h"
#include "line_index.h"

namespace mxy {

// sort_hits.hip
hipError_t sort_pairs(unsigned long long* keys, uint32_t* vals, uint32_t n, void* temp, size_t temp_bytes, hipStream_t stream);
const uint32_t* sort_pairs_half(const void* temp);

namespace {

namespace X = xrender;

constexpr uint32_t XR_THREADS = 256, XR_WAVES = XR_THREADS / 64;
constexpr uint32_t XR_KEY_ITEMS = XR_KEY_TILE / XR_THREADS, XR_ITEMS = XR_SCAN_CHUNK / XR_THREADS;
constexpr uint32_t XR_STAGE = 8192;            // bytes of the block a wave stages in LDS per turn (k_xr_write_short)
constexpr uint64_t XR_LONG_BIT = 1ull << 63;   // in rec_len: the record is on the long list (not part of its length)
static_assert(XR_KEY_TILE % XR_THREADS == 0 && XR_SCAN_CHUNK % XR_THREADS == 0, "whole entries per thread");
static_assert(XR_STAGE % 1024 == 0, "whole 16-byte stores of 64 lanes");
static_assert(XR_KEY_ITEMS <= 32, "one bit per item");
using TypeAgg = LdsAggregator<5, 4, 4>;        // key = item type: twelve of them, and whatever a foreign list carries

__device__ __forceinline__ uint32_t lane() { return __lane_id(); }
__device__ __forceinline__ uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t wave_incl(uint32_t v) {
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off);
        if (lane() >= off) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_last(uint32_t incl) { return __shfl(incl, 63); }
// the lanes of a wave have written LDS that other lanes of the same wave read next (and the other way round)
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------ candidates
struct Cand { uint32_t start, len, type; bool real; };
// entry idx of the two lists, inside the batch whatever it says (in.len > 0 where a list has a real entry)
__device__ __forceinline__ Cand load_cand(const XrInput& in, uint32_t idx) {
    const uint4 v = *reinterpret_cast<const uint4*>(idx < in.n_a ? in.list_a + idx : in.list_b + (idx - in.n_a));
    Cand c;
    c.real = v.y != 0xFFFFFFFFu && in.len != 0;
    c.start = min(v.x, in.len ? in.len - 1u : 0u);
    c.len = min(v.y & 0xFFFFFFu, in.len - c.start);
    c.type = v.y >> 24;
    return c;
}

// '\n' bytes of [tile start, s), s < len: whole 16-byte words, and the bytes of the last word in front of s under a mask
__device__ __forceinline__ uint32_t nl_before(const uint8_t* __restrict__ data, uint32_t len, uint32_t s) {
    const uint32_t base = s & ~(LINE_TILE - 1u), r = s - base;
    uint32_t cnt = 0;
    for (uint32_t w = 0; w * 16u < r; ++w) {   // bound: LINE_TILE / 16
        const uint32_t off = base + w * 16u, nb = min(r - w * 16u, 16u);   // bytes of this word that count
        uint32_t x[4] = {0, 0, 0, 0};
        if (off + 16u <= len) {
            const uint4 v = *reinterpret_cast<const uint4*>(data + off);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            for (uint32_t k = 0; k < nb; ++k) x[k >> 2] |= (uint32_t)data[off + k] << (8u * (k & 3u));   // off + k < s < len
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t have = nb > 4u * j ? min(nb - 4u * j, 4u) : 0u;
            const uint32_t mask = have >= 4u ? 0xFFFFFFFFu : (1u << (8u * have)) - 1u;
            cnt += __popc(nl_bytes(x[j]) & mask & 0x80808080u);
        }
    }
    return cnt;
}

// ------------------------------------------------------------------------------------------------ keys
__global__ __launch_bounds__(XR_THREADS) void k_xr_keys(XrInput in, XrWork w) {
    __shared__ uint32_t agg_keys[TypeAgg::SLOTS], agg_counts[TypeAgg::SLOTS];
    __shared__ uint32_t cnt[XR_KEY_ITEMS][XR_WAVES];
    __shared__ uint32_t tile_base;
    const uint32_t n_list = in.n_a + in.n_b, wave = threadIdx.x >> 6;
    const uint64_t lt = (1ull << lane()) - 1ull;
    TypeAgg::clear(agg_keys, agg_counts, XR_THREADS);
    __syncthreads();
    unsigned long long key[XR_KEY_ITEMS];
    uint32_t rank_in_wave[XR_KEY_ITEMS], real_bits = 0;
#pragma unroll
    for (uint32_t r = 0; r < XR_KEY_ITEMS; ++r) {
        const uint32_t idx = blockIdx.x * XR_KEY_TILE + r * XR_THREADS + threadIdx.x;   // the grid covers n_list < 2^32 entries
        Cand c{0, 0, 0, false};
        key[r] = 0;
        if (idx < n_list) c = load_cand(in, idx);
        if (c.real) key[r] = X::key_pack(w.line_prefix[c.start / LINE_TILE] + nl_before(in.data, in.len, c.start), X::rank(c.type), c.start);
        const uint64_t m = __ballot(c.real);
        rank_in_wave[r] = (uint32_t)__popcll(m & lt);
        if (lane() == 0) cnt[r][wave] = (uint32_t)__popcll(m);
        if (c.real) real_bits |= 1u << r;
        const uint32_t over = TypeAgg::count(agg_keys, agg_counts, m, c.type, lane());
        if (over && c.type < IT_COUNT) atomicAdd(&w.ctr->by_type[c.type].n, over);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t r = 0; r < XR_KEY_ITEMS; ++r) for (uint32_t v = 0; v < XR_WAVES; ++v) total += cnt[r][v];
        tile_base = total ? atomicAdd(&w.ctr->pairs.n_pairs, total) : 0u;   // counts past the capacity
    }
    __syncthreads();
    uint32_t run = tile_base;
#pragma unroll
    for (uint32_t r = 0; r < XR_KEY_ITEMS; ++r) {
#pragma unroll
        for (uint32_t v = 0; v < XR_WAVES; ++v) {
            if (v == wave && ((real_bits >> r) & 1u)) {
                const uint32_t slot = run + rank_in_wave[r];
                if (slot < in.n_real) {
                    w.keys[slot] = key[r];
                    w.vals[slot] = blockIdx.x * XR_KEY_TILE + r * XR_THREADS + threadIdx.x;
                }
            }
            run += cnt[r][v];
        }
    }
    TypeAgg::flush(agg_keys, agg_counts, XR_THREADS, [&](uint32_t type, uint32_t c) { if (type < IT_COUNT) atomicAdd(&w.ctr->by_type[type].n, c); });
}

// ------------------------------------------------------------------------------------------------ measure
// the sorted records: pairs_n of them, their list indices in the half the sort left them in
struct Sorted { uint32_t n; const uint32_t* vals; };
__device__ __forceinline__ Sorted sorted_of(const XrInput& in, const XrWork& w) {
    Sorted s;
    s.n = min(w.ctr->pairs.n_pairs, in.n_real);
    s.vals = w.vals + (size_t)(s.n ? *w.sort_half : 0u) * in.n_real;
    return s;
}

// escapes of f[0, n): four bytes per load while four are left (an unaligned load inside the candidate), then byte by byte
__device__ __forceinline__ uint32_t escapes_lane(uint32_t format, const uint8_t* __restrict__ f, uint32_t n) {
    if (format == X::FORMAT_TEXT) return 0;
    uint32_t e = 0, i = 0;
    for (; i + 4u <= n; i += 4u) {   // bound: XR_SHORT_MAX / 4
        uint32_t x;
        __builtin_memcpy(&x, f + i, 4);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) e += X::is_escape(format, (uint8_t)(x >> (8u * k)));
    }
    for (; i < n; ++i) e += X::is_escape(format, f[i]);   // bound: 3
    return e;
}

__global__ __launch_bounds__(XR_THREADS) void k_xr_measure(XrInput in, XrWork w) {
    const Sorted s = sorted_of(in, w);
    const uint32_t i = blockIdx.x * XR_THREADS + threadIdx.x, n_list = in.n_a + in.n_b;
    if (i >= s.n) return;
    const uint32_t idx = s.vals[i];
    if (idx >= n_list) { w.rec_len[i] = 0; return; }   // never, for pairs k_xr_keys wrote
    const Cand c = load_cand(in, idx);
    if (c.len <= XR_SHORT_MAX) {
        w.rec_len[i] = X::record_len(in.format, c.type, c.len, escapes_lane(in.format, in.data + c.start, c.len));
        return;
    }
    const uint32_t slot = atomicAdd(&w.ctr->longs.n_long, 1u);   // few: long candidates are rare
    if (slot < in.n_real) w.long_list[slot] = i;
    w.rec_len[i] = XR_LONG_BIT;
}

__global__ __launch_bounds__(XR_THREADS) void k_xr_long_measure(XrInput in, XrWork w) {
    const Sorted s = sorted_of(in, w);
    const uint32_t n_long = min(w.ctr->longs.n_long, in.n_real), n_list = in.n_a + in.n_b;
    const uint32_t wave = blockIdx.x * XR_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * XR_WAVES;
    for (uint32_t li = wave; li < n_long; li += n_waves) {   // bound: the long list
        const uint32_t i = w.long_list[li];
        if (i >= s.n) continue;
        const uint32_t idx = s.vals[i];
        if (idx >= n_list) continue;
        const Cand c = load_cand(in, idx);
        uint64_t esc = 0;
        for (uint32_t base = 0; base < c.len; base += 64u) {   // bound: 2^24 / 64
            const uint32_t k = base + lane();
            esc += (uint64_t)__popcll(__ballot(k < c.len && X::is_escape(in.format, in.data[c.start + k])));
        }
        if (lane() == 0) w.rec_len[i] = X::record_len(in.format, c.type, c.len, esc) | XR_LONG_BIT;
    }
}

// ------------------------------------------------------------------------------------------------ offsets
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* s) {
#pragma unroll
    for (uint32_t off = 32; off; off >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, off);
    if (lane() == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < XR_WAVES; ++k) t += s[k];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(XR_THREADS) void k_xr_chunk_sum(XrInput in, XrWork w) {
    __shared__ uint64_t s[XR_WAVES];
    const uint32_t n = min(w.ctr->pairs.n_pairs, in.n_real), first = blockIdx.x * XR_SCAN_CHUNK;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < XR_ITEMS; ++r) {
        const uint32_t i = first + r * XR_THREADS + threadIdx.x;
        if (i < n) v += w.rec_len[i] & ~XR_LONG_BIT;
    }
    v = block_sum(v, s);
    if (threadIdx.x == 0) w.chunk_sums[blockIdx.x] = v;
}

// rec_off[i] = sum of the lengths in front of record i, i = 0 .. n; the total is the demand
__global__ __launch_bounds__(XR_THREADS) void k_xr_scan(XrInput in, XrWork w) {
    __shared__ uint64_t s[XR_THREADS];
    __shared__ uint64_t sw[XR_WAVES];
    const uint32_t n = min(w.ctr->pairs.n_pairs, in.n_real);
    if (blockIdx.x == 0 && threadIdx.x == 0 && w.ctr->pairs.n_pairs != in.n_real) w.ctr->out.status = XR_MISCOUNT;
    if (n == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { w.rec_off[0] = 0; w.ctr->out.demand = 0; }
        return;
    }
    uint64_t before = 0;
    for (uint32_t c = threadIdx.x; c < blockIdx.x; c += XR_THREADS) before += w.chunk_sums[c];   // bound: the chunks in front
    before = block_sum(before, sw);
    const uint32_t i0 = blockIdx.x * XR_SCAN_CHUNK + threadIdx.x * XR_ITEMS;
    uint64_t c[XR_ITEMS], own = 0;
#pragma unroll
    for (uint32_t r = 0; r < XR_ITEMS; ++r) { c[r] = i0 + r < n ? w.rec_len[i0 + r] & ~XR_LONG_BIT : 0ull; own += c[r]; }
    s[threadIdx.x] = own;
    __syncthreads();
    uint64_t incl = own;
    for (uint32_t off = 1; off < XR_THREADS; off <<= 1) {
        const uint64_t v = threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
        __syncthreads();
        incl += v;
        s[threadIdx.x] = incl;
        __syncthreads();
    }
    uint64_t run = before + incl - own;
#pragma unroll
    for (uint32_t r = 0; r < XR_ITEMS; ++r) {
        if (i0 + r < n) w.rec_off[i0 + r] = run;
        run += c[r];
        if (i0 + r + 1 == n) { w.rec_off[n] = run; w.ctr->out.demand = run; }
    }
}

// ------------------------------------------------------------------------------------------------ write
// A lane's record into the window [w0, w0 + XR_STAGE) of the block that its wave stages in LDS; bytes outside the window are dropped.
struct StageSink {
    uint8_t* lds;
    uint64_t pos, w0;
    __device__ __forceinline__ void put(const uint8_t* p, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) { const uint64_t q = pos + k - w0; if (pos + k >= w0 && q < XR_STAGE) lds[q] = p[k]; }   // bound: len
        pos += len;
    }
};

// Short records. The records of a wave's 64 lanes lie side by side in the block (a long record among them is a hole that
// k_xr_write_long fills), so the wave takes each run of consecutive short records as one range of the block: window by window of
// XR_STAGE bytes, every lane of the run puts what its record has inside the window into LDS, then the wave stores the window — the bytes
// up to the block's next 16-byte boundary and the ragged end one byte per lane, the body as 16-byte stores, contiguous over the lanes.
// No store at or behind min(demand, capacity).
__global__ __launch_bounds__(XR_THREADS) void k_xr_write_short(XrInput in, XrWork w, uint8_t* __restrict__ text, uint64_t capacity) {
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[XR_WAVES][XR_STAGE];
    if (w.ctr->out.status != XR_OK) return;
    const Sorted s = sorted_of(in, w);
    uint8_t* stage = stage_all[threadIdx.x >> 6];
    const uint32_t i = blockIdx.x * XR_THREADS + threadIdx.x, n_list = in.n_a + in.n_b;
    const uint64_t end = min64(w.ctr->out.demand, capacity);   // no store at or behind it
    uint64_t lo = 0, hi = 0;
    bool mine = false;
    Cand c{0, 0, 0, false};
    if (i < s.n) {
        const uint64_t len = w.rec_len[i];
        const uint32_t idx = s.vals[i];
        mine = !(len & XR_LONG_BIT) && idx < n_list;
        if (mine) { lo = w.rec_off[i]; hi = lo + len; c = load_cand(in, idx); }
    }
    unsigned long long left = __ballot(mine);
    while (left) {   // bound: the runs of short records among 64 lanes, at most 32
        const uint32_t a = (uint32_t)__ffsll((long long)left) - 1u;
        const unsigned long long gap = ~(left >> a);   // bit k: lane a + k is not short
        const uint32_t b = gap ? a + (uint32_t)__ffsll((long long)gap) - 1u : 64u;   // the run is lanes a .. b - 1
        left &= b >= 64u ? 0ull : ~0ull << b;
        const uint64_t run_lo = (uint64_t)__shfl((unsigned long long)lo, (int)a);
        const uint64_t run_hi = min64((uint64_t)__shfl((unsigned long long)hi, (int)(b - 1u)), end);
        const bool in_run = lane() >= a && lane() < b;
        if (run_lo >= run_hi) continue;   // the run begins at or behind the end (a block that is too small): nothing of it is stored
        for (uint64_t w0 = run_lo & ~15ull; w0 < run_hi; w0 += XR_STAGE) {   // bound: the text of at most 64 short records / XR_STAGE
            if (in_run && hi > w0 && lo < w0 + XR_STAGE) {
                StageSink sink{stage, lo, w0};
                uint8_t t[X::HEAD_MAX];
                sink.put(t, X::head_put(in.format, c.type, t));
                const uint8_t* f = in.data + c.start;
                for (uint32_t k = 0; k < c.len; ++k) sink.put(t, X::byte_put(in.format, f[k], t));   // bound: XR_SHORT_MAX
                sink.put(t, X::tail_put(in.format, t));
            }
            wave_sync_lds();
            const uint64_t f_lo = run_lo > w0 ? run_lo : w0, f_hi = min64(run_hi, w0 + XR_STAGE);
            const uint64_t head_end = min64(f_hi, (f_lo + 15ull) & ~15ull);   // at most 15 bytes
            if (f_lo + lane() < head_end) text[f_lo + lane()] = stage[f_lo + lane() - w0];
            const uint64_t body_end = f_hi & ~15ull;
            for (uint64_t p = head_end + lane() * 16ull; p + 16ull <= body_end; p += 64ull * 16ull)   // bound: XR_STAGE / 1024 steps
                *reinterpret_cast<uint4*>(text + p) = *reinterpret_cast<const uint4*>(stage + (p - w0));
            const uint64_t tail = body_end > head_end ? body_end : head_end;   // at most 15 bytes
            if (tail + lane() < f_hi) text[tail + lane()] = stage[tail + lane() - w0];
            wave_sync_lds();
        }
    }
}

__global__ __launch_bounds__(XR_THREADS) void k_xr_write_long(XrInput in, XrWork w, uint8_t* __restrict__ text, uint64_t capacity) {
    if (w.ctr->out.status != XR_OK) return;
    const Sorted s = sorted_of(in, w);
    const uint32_t n_long = min(w.ctr->longs.n_long, in.n_real), n_list = in.n_a + in.n_b;
    const uint64_t end = min64(w.ctr->out.demand, capacity);   // no store at or behind it
    const uint32_t wave = blockIdx.x * XR_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * XR_WAVES;
    for (uint32_t li = wave; li < n_long; li += n_waves) {   // bound: the long list
        const uint32_t i = w.long_list[li];
        if (i >= s.n) continue;
        const uint32_t idx = s.vals[i];
        uint64_t pos = w.rec_off[i];
        if (idx >= n_list || pos >= end) continue;
        const Cand c = load_cand(in, idx);
        uint8_t t[X::HEAD_MAX];
        const uint32_t nh = X::head_put(in.format, c.type, t);
        if (lane() == 0) for (uint32_t k = 0; k < nh; ++k) if (pos + k < end) text[pos + k] = t[k];   // bound: HEAD_MAX
        pos += nh;
        for (uint32_t base = 0; base < c.len; base += 64u) {   // bound: 2^24 / 64
            const uint32_t k = base + lane();
            const uint32_t nb = k < c.len ? X::byte_put(in.format, in.data[c.start + k], t) : 0u;
            const uint32_t incl = wave_incl(nb);
            for (uint32_t j = 0; j < nb; ++j) if (pos + incl - nb + j < end) text[pos + incl - nb + j] = t[j];   // bound: 2
            pos += wave_last(incl);
        }
        const uint32_t nt = X::tail_put(in.format, t);
        if (lane() == 0) for (uint32_t k = 0; k < nt; ++k) if (pos + k < end) text[pos + k] = t[k];   // bound: TAIL_MAX
    }
}

uint32_t long_grid(uint32_t n, int n_cu) { return std::min<uint32_t>((n + XR_WAVES - 1) / XR_WAVES, (uint32_t)std::max(n_cu, 1) * 4u); }

}  // namespace

const uint32_t* xr_sort_half(const void* sort_temp) { return sort_pairs_half(sort_temp); }
uint32_t xr_chunks(uint32_t n) { return std::max<uint32_t>(1u, (uint32_t)(((uint64_t)n + XR_SCAN_CHUNK - 1) / XR_SCAN_CHUNK)); }

static bool launch_fits(const XrInput& in) {
    return in.len <= X::MAX_LEN && (uint64_t)in.n_a + in.n_b <= 0xFFFFFFFFull && in.format < X::FORMAT_COUNT && !(reinterpret_cast<uintptr_t>(in.data) & 15u);
}

hipError_t extract_render_order(const XrInput& in, const XrWork& w, int n_cu, hipStream_t stream) {
    if (!launch_fits(in)) return hipErrorInvalidValue;
    const uint32_t n_list = in.n_a + in.n_b;
    if (!n_list) return hipSuccess;   // the counters stay zero
    hipError_t e = line_index_build(in.data, in.len, w.line_counts, w.line_chunks, w.line_prefix, n_cu, stream, nullptr);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_xr_keys, dim3((uint32_t)(((uint64_t)n_list + XR_KEY_TILE - 1) / XR_KEY_TILE)), dim3(XR_THREADS), 0, stream, in, w);
    e = sort_pairs(w.keys, w.vals, in.n_real, w.sort_temp, w.sort_temp_bytes, stream);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t extract_render_measure(const XrInput& in, const XrWork& w, int n_cu, hipStream_t stream) {
    if (!launch_fits(in)) return hipErrorInvalidValue;
    const uint32_t n = in.n_real;
    if (n) {
        hipLaunchKernelGGL(k_xr_measure, dim3((n + XR_THREADS - 1) / XR_THREADS), dim3(XR_THREADS), 0, stream, in, w);
        // few records are long: the workgroups leave at once where the list is empty
        hipLaunchKernelGGL(k_xr_long_measure, dim3(long_grid(n, n_cu)), dim3(XR_THREADS), 0, stream, in, w);
    }
    hipLaunchKernelGGL(k_xr_chunk_sum, dim3(xr_chunks(n)), dim3(XR_THREADS), 0, stream, in, w);
    hipLaunchKernelGGL(k_xr_scan, dim3(xr_chunks(n)), dim3(XR_THREADS), 0, stream, in, w);
    return hipGetLastError();
}

hipError_t extract_render_write(const XrInput& in, const XrWork& w, uint8_t* text, uint64_t capacity, int n_cu, hipStream_t stream) {
    if (!launch_fits(in)) return hipErrorInvalidValue;
    const uint32_t n = in.n_real;
    if (!n || !capacity) return hipSuccess;   // nothing may be stored; the demand is counted by extract_render_measure
    if (reinterpret_cast<uintptr_t>(text) & 15u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_xr_write_short, dim3((n + XR_THREADS - 1) / XR_THREADS), dim3(XR_THREADS), 0, stream, in, w, text, capacity);
    hipLaunchKernelGGL(k_xr_write_long, dim3(long_grid(n, n_cu)), dim3(XR_THREADS), 0, stream, in, w, text, capacity);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
template <class Buf>
void ExtractRender::grow(Buf& b, size_t want, size_t room) {
    if (b.n >= want && b.p) return;
    b.alloc(want + room);
    ++allocations_;
}

XrWork ExtractRender::work() const {
    XrWork w{};
    w.line_counts = line_counts_.p; w.line_chunks = line_chunks_.p; w.line_prefix = line_prefix_.p;
    w.keys = keys_.p; w.vals = vals_.p; w.sort_temp = sort_tmp_.p; w.sort_temp_bytes = sort_tmp_.n; w.sort_half = xr_sort_half(sort_tmp_.p);
    w.rec_len = rec_len_.p; w.rec_off = rec_off_.p; w.chunk_sums = chunks_.p; w.long_list = long_list_.p;
    w.ctr = ctr_.p;
    return w;
}

void ExtractRender::resolve(const XrInput& in, int n_cu, hipStream_t stream) {
    in_ = in; n_cu_ = n_cu; stream_ = stream; refused_ = false;
    queued_ = (uint64_t)in.n_a + in.n_b != 0 && in.n_real != 0;
    for (float& m : ms_) m = 0;
    if (!queued_) return;
    if (!launch_fits(in)) throw HipError{"extract render: the launch is larger than the order key holds"};
    const size_t n = in.n_real, tiles = line_tiles(in.len);
    grow(line_counts_, tiles, tiles / 4 + 1024);
    grow(line_prefix_, tiles + 1, tiles / 4 + 1024);
    grow(line_chunks_, line_chunks((uint32_t)tiles), 64);
    grow(keys_, 2 * n, n / 2 + 4096);
    grow(vals_, 2 * n, n / 2 + 4096);
    grow(sort_tmp_, sort_hits_temp_bytes((uint32_t)n), sort_hits_temp_bytes((uint32_t)n) / 4 + 4096);
    grow(rec_len_, n, n / 4 + 1024);
    grow(rec_off_, n + 1, n / 4 + 1024);
    grow(long_list_, n, n / 4 + 1024);
    grow(chunks_, xr_chunks((uint32_t)n), 64);
    grow(ctr_, 1, 0);
    // the first block of a scanner: 64 bytes per record; afterwards what the scans before left
    grow(text_, 1, n * 64 + 4096);
    if (!pinned_ctr_.p) { pinned_ctr_.alloc(1); ++allocations_; }
    for (Event& e : ev_) e.create();
    const XrWork w = work();
    MXY_HIP(hipEventRecord(ev_[0], stream));
    MXY_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(XrCounters), stream));
    MXY_HIP(extract_render_order(in, w, n_cu, stream));
    MXY_HIP(hipEventRecord(ev_[1], stream));
    MXY_HIP(extract_render_measure(in, w, n_cu, stream));
    MXY_HIP(hipEventRecord(ev_[2], stream));
    MXY_HIP(extract_render_write(in, w, text_.p, text_.n, n_cu, stream));
    MXY_HIP(hipEventRecord(ev_[3], stream));
    MXY_HIP(hipMemcpyAsync(pinned_ctr_.p, ctr_.p, sizeof(XrCounters), hipMemcpyDeviceToHost, stream));
}

ExtractTextView ExtractRender::finish() {
    ExtractTextView v;
    v.armed = true;
    if (refused_) { refused_ = false; v.status = XR_REFUSED; return v; }
    if (!queued_) return v;
    queued_ = false;
    const XrCounters& c = *pinned_ctr_.p;
    MXY_HIP(hipEventElapsedTime(&ms_[0], ev_[0], ev_[1]));
    MXY_HIP(hipEventElapsedTime(&ms_[1], ev_[1], ev_[2]));
    MXY_HIP(hipEventElapsedTime(&ms_[2], ev_[2], ev_[3]));
    v.status = c.out.status;
    if (v.status != XR_OK) return v;
    v.n_records = c.pairs.n_pairs;
    for (int t = 0; t < IT_COUNT; ++t) v.by_type[t] = c.by_type[t].n;
    v.len = c.out.demand;
    if (!v.len) return v;
    if (v.len > text_.n) {   // the block was too small: the demand is exact, so one regrow settles it, and only the write step runs again
        grow(text_, (size_t)v.len, (size_t)v.len / 4 + 4096);
        MXY_HIP(hipEventRecord(ev_[2], stream_));
        MXY_HIP(extract_render_write(in_, work(), text_.p, text_.n, n_cu_, stream_));
        MXY_HIP(hipEventRecord(ev_[3], stream_));
        MXY_HIP(hipStreamSynchronize(stream_));
        MXY_HIP(hipEventElapsedTime(&ms_[2], ev_[2], ev_[3]));
    }
    // behind the blocks of the pieces in front: a pinned block that is too small is replaced by a larger one that keeps them
    if (pinned_text_.n < joined_len_ + v.len) {
        PinnedBuf<uint8_t> larger;
        const size_t want = (size_t)(joined_len_ + v.len);
        larger.alloc(want + want / 4 + (1 << 16));
        ++allocations_;
        if (joined_len_) memcpy(larger.p, pinned_text_.p, (size_t)joined_len_);
        std::swap(larger.p, pinned_text_.p);
        std::swap(larger.n, pinned_text_.n);
    }
    MXY_HIP(hipEventRecord(ev_[4], stream_));
    MXY_HIP(hipMemcpyAsync(pinned_text_.p + joined_len_, text_.p, (size_t)v.len, hipMemcpyDeviceToHost, stream_));
    MXY_HIP(hipEventRecord(ev_[5], stream_));
    MXY_HIP(hipStreamSynchronize(stream_));
    MXY_HIP(hipEventElapsedTime(&ms_[3], ev_[4], ev_[5]));
    v.text = pinned_text_.p + joined_len_;
    joined_len_ += v.len;
    return v;
}

}  // namespace mxy
