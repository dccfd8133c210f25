// Hit lines, on the GPU: the distinct lines that contain at least one hit, packed into one contiguous block in ascending line order,
// each ended by one '\n', so that a caller who renders records fetches those lines and not the batch. Everything it needs lies in
// device memory behind LineContext::resolve — a LineRec{line, line_start, line_end} per record — and the host knows the '\n' count:
//   k_hl_mark        one lane per record: atomicOr into a bitmap with one bit per line of the batch
//   k_hl_chunk_sum   } exclusive prefix of the words' popcounts (the shape of k_line_chunk_sum / k_line_scan): the rank of a line is
//   k_hl_scan        } word_prefix[line >> 5] + popc(the word's bits below the line's); the total is the number of distinct lines
//   k_hl_lengths     one lane per record: line_of[i] = rank, and src / len / line_no of the line at [rank]. Every record of a line
//                    stores them — they carry the same start and end, so the values are the same and no winner flag is kept
//   k_hl_chunk_sum   } exclusive prefix of len[] into line_off[0 .. n_lines] (the count is read on the device); the last entry is
//   k_hl_scan        } the demand of the block
//   k_hl_copy        partitioned by OUTPUT: a wave owns HIT_LINES_SLICE bytes of the block, searches line_off once for the first line
//                    that reaches into them and copies what intersects them. A line of 40 MB is spread over ten thousand waves, a run
//                    of 20-byte lines costs a wave one search. Stores are contiguous per wave and 16 bytes wide behind the first
//                    16-byte boundary of a piece; the source is read with aligned 16-byte loads and shifted into place where its
//                    alignment differs, and the ragged ends go byte by byte.
// Every store sits behind a bound: the bitmap behind n_bits, the per-line arrays behind the record count, the block behind
// min(demand, capacity). No load of log bytes reaches `len` (the rule of k_line_resolve).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hit_lines.h"

namespace mxy {

namespace {

constexpr uint32_t HL_THREADS = 256, HL_WAVES = HL_THREADS / 64;
constexpr uint32_t HL_ITEMS = HIT_LINES_SCAN_CHUNK / HL_THREADS;
constexpr uint32_t HL_GROUP = 16;   // lanes that share a line where a slice holds several
static_assert(HIT_LINES_SCAN_CHUNK % HL_THREADS == 0, "whole entries per thread");
static_assert(HIT_LINES_SLICE % 16 == 0, "a slice begins at a 16-byte boundary of the block");

__device__ __forceinline__ LineRec record_line(const LineRec* __restrict__ fin_lines, uint32_t n_fin, const LineRec* __restrict__ c4_lines, uint32_t i) {
    const uint4 v = *reinterpret_cast<const uint4*>(i < n_fin ? fin_lines + i : c4_lines + (i - n_fin));
    return LineRec{v.x, v.y, v.z, v.w};
}

__global__ __launch_bounds__(HL_THREADS) void k_hl_mark(const LineRec* __restrict__ fin_lines, uint32_t n_fin, const LineRec* __restrict__ c4_lines, uint32_t n,
                                                        uint32_t* __restrict__ bitmap, uint32_t n_bits) {
    const uint32_t i = blockIdx.x * HL_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t line = record_line(fin_lines, n_fin, c4_lines, i).line;
    if (line < n_bits) atomicOr(&bitmap[line >> 5], 1u << (line & 31u));
}

// what the two prefix sums add up
struct PopcOf { const uint32_t* w; __device__ __forceinline__ uint32_t operator()(uint32_t t) const { return (uint32_t)__popc(w[t]); } };
struct ValueOf { const uint32_t* v; __device__ __forceinline__ uint32_t operator()(uint32_t t) const { return v[t]; } };

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s) {
    for (uint32_t off = 32; off; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63u) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (uint32_t w = 0; w < HL_WAVES; ++w) t += s[w];
    __syncthreads();
    return t;
}

// n entries: n_dev ? *n_dev : n_host (the grid covers the host's bound; a workgroup behind the count sums nothing)
template <class V>
__global__ __launch_bounds__(HL_THREADS) void k_hl_chunk_sum(V val, uint32_t n_host, const uint32_t* __restrict__ n_dev, uint32_t* __restrict__ chunk_sums) {
    __shared__ uint32_t s[HL_WAVES];
    const uint32_t n = n_dev ? min(*n_dev, n_host) : n_host;
    const uint32_t first = blockIdx.x * HIT_LINES_SCAN_CHUNK;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t r = 0; r < HL_ITEMS; ++r) {
        const uint32_t t = first + r * HL_THREADS + threadIdx.x;
        if (t < n) v += val(t);
    }
    v = block_sum(v, s);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = v;
}

// prefix[t] = sum of the entries in front of t, t = 0 .. n; the total also goes to *total
template <class V>
__global__ __launch_bounds__(HL_THREADS) void k_hl_scan(V val, uint32_t n_host, const uint32_t* __restrict__ n_dev, const uint32_t* __restrict__ chunk_sums,
                                                        uint32_t* __restrict__ prefix, uint32_t* __restrict__ total) {
    __shared__ uint32_t s[HL_THREADS];
    __shared__ uint32_t sw[HL_WAVES];
    const uint32_t n = n_dev ? min(*n_dev, n_host) : n_host;
    if (n == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { prefix[0] = 0; *total = 0; }
        return;
    }
    uint32_t before = 0;
    for (uint32_t c = threadIdx.x; c < blockIdx.x; c += HL_THREADS) before += chunk_sums[c];
    before = block_sum(before, sw);
    const uint32_t t0 = blockIdx.x * HIT_LINES_SCAN_CHUNK + threadIdx.x * HL_ITEMS;
    uint32_t c[HL_ITEMS], own = 0;
#pragma unroll
    for (uint32_t r = 0; r < HL_ITEMS; ++r) { c[r] = t0 + r < n ? val(t0 + r) : 0u; own += c[r]; }
    s[threadIdx.x] = own;
    __syncthreads();
    uint32_t incl = own;   // inclusive prefix over the threads' sums
    for (uint32_t off = 1; off < HL_THREADS; off <<= 1) {
        const uint32_t t = threadIdx.x >= off ? s[threadIdx.x - off] : 0u;
        __syncthreads();
        incl += t;
        s[threadIdx.x] = incl;
        __syncthreads();
    }
    uint32_t run = before + incl - own;
#pragma unroll
    for (uint32_t r = 0; r < HL_ITEMS; ++r) {
        if (t0 + r < n) prefix[t0 + r] = run;
        run += c[r];
        if (t0 + r + 1 == n) { prefix[n] = run; *total = run; }
    }
}

__global__ __launch_bounds__(HL_THREADS) void k_hl_lengths(const LineRec* __restrict__ fin_lines, uint32_t n_fin, const LineRec* __restrict__ c4_lines, uint32_t n,
                                                           const uint32_t* __restrict__ bitmap, uint32_t n_bits, const uint32_t* __restrict__ word_prefix,
                                                           uint32_t* __restrict__ src, uint32_t* __restrict__ len, uint32_t* __restrict__ line_no,
                                                           uint32_t* __restrict__ line_of) {
    const uint32_t i = blockIdx.x * HL_THREADS + threadIdx.x;
    if (i >= n) return;
    const LineRec r = record_line(fin_lines, n_fin, c4_lines, i);
    uint32_t rank = 0xFFFFFFFFu;
    if (r.line < n_bits) rank = word_prefix[r.line >> 5] + (uint32_t)__popc(bitmap[r.line >> 5] & ((1u << (r.line & 31u)) - 1u));
    line_of[i] = rank;
    if (rank < n) {   // distinct lines never outnumber the records
        src[rank] = r.line_start;
        len[rank] = r.line_end - r.line_start + 1u;   // the '\n' the block ends the line with
        line_no[rank] = r.line;
    }
}

// 16 bytes at `off` (a multiple of 16; `data` is 16-byte aligned); bytes at or behind `len` read as zero and are not touched
__device__ __forceinline__ uint4 load16(const uint8_t* __restrict__ data, uint32_t off, uint32_t len) {
    if (off + 16u <= len) return *reinterpret_cast<const uint4*>(data + off);
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < 16u; ++k)
        if (off + k < len) w[k >> 2] |= (uint32_t)data[off + k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// dword at byte `bs` (0..3) of hi:lo
__device__ __forceinline__ uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t bs) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * bs)); }

// bytes sh .. sh + 15 of the 32 bytes a:b, 0 < sh < 16 (sh is uniform over the lanes of a piece: the branch does not diverge)
__device__ __forceinline__ uint4 shifted16(uint4 a, uint4 b, uint32_t sh) {
    const uint32_t bs = sh & 3u;
    switch (sh >> 2) {
    case 0: return make_uint4(align_bytes(a.y, a.x, bs), align_bytes(a.z, a.y, bs), align_bytes(a.w, a.z, bs), align_bytes(b.x, a.w, bs));
    case 1: return make_uint4(align_bytes(a.z, a.y, bs), align_bytes(a.w, a.z, bs), align_bytes(b.x, a.w, bs), align_bytes(b.y, b.x, bs));
    case 2: return make_uint4(align_bytes(a.w, a.z, bs), align_bytes(b.x, a.w, bs), align_bytes(b.y, b.x, bs), align_bytes(b.z, b.y, bs));
    default: return make_uint4(align_bytes(b.x, a.w, bs), align_bytes(b.y, b.x, bs), align_bytes(b.z, b.y, bs), align_bytes(b.w, b.z, bs));
    }
}

// text[p_lo, p_hi) = data[q_lo ..), by the `width` lanes sub = 0 .. width - 1 (width >= 16). The caller has clipped the range to its
// slice and to the capacity, and data[q_lo + (p_hi - p_lo)) still lies inside the line, hence inside the batch.
__device__ __forceinline__ void copy_piece(const uint8_t* __restrict__ data, uint32_t data_len, uint8_t* __restrict__ text, uint32_t p_lo, uint32_t p_hi,
                                           uint32_t q_lo, uint32_t sub, uint32_t width) {
    const uint32_t head_end = min(p_hi, (p_lo + 15u) & ~15u);   // up to the first 16-byte boundary of the block: at most 15 bytes
    if (sub < head_end - p_lo) text[p_lo + sub] = data[q_lo + sub];
    const uint32_t body_end = p_hi & ~15u;
    if (body_end <= head_end) {   // no whole 16 bytes: the head was everything, or a tail of at most 15 bytes is left
        if (head_end < p_hi && sub < p_hi - head_end) text[head_end + sub] = data[q_lo + (head_end - p_lo) + sub];
        return;
    }
    const uint32_t q0 = q_lo + (head_end - p_lo), sh = q0 & 15u;
    for (uint32_t p = head_end + sub * 16u; p < body_end; p += width * 16u) {
        const uint32_t a = q0 - sh + (p - head_end);   // a + 16 <= q + 16 <= the line's end <= data_len
        uint4 v = *reinterpret_cast<const uint4*>(data + a);
        if (sh) v = shifted16(v, load16(data, a + 16u, data_len), sh);   // of the second load only bytes in front of q + 16 are used
        *reinterpret_cast<uint4*>(text + p) = v;
    }
    if (sub < p_hi - body_end) text[body_end + sub] = data[q_lo + (body_end - p_lo) + sub];
}

// line k of the block (bytes [o0, o1), the last one its terminator) as far as it lies in [s0, s1)
__device__ __forceinline__ void copy_line(const uint8_t* __restrict__ data, uint32_t data_len, uint8_t* __restrict__ text, uint32_t line_src, uint32_t o0, uint32_t o1,
                                          uint32_t s0, uint32_t s1, uint32_t sub, uint32_t width) {
    const uint32_t term = o1 - 1u;
    const uint32_t p_lo = max(o0, s0), p_hi = min(term, s1);
    if (p_lo < p_hi) copy_piece(data, data_len, text, p_lo, p_hi, line_src + (p_lo - o0), sub, width);
    if (sub == 0 && term >= s0 && term < s1) text[term] = '\n';
}

__global__ __launch_bounds__(HL_THREADS) void k_hl_copy(const uint8_t* __restrict__ data, uint32_t data_len, const HitLineCounters* __restrict__ ctr,
                                                        const uint32_t* __restrict__ src, const uint32_t* __restrict__ line_off, uint8_t* __restrict__ text,
                                                        uint32_t capacity) {
    const uint32_t n_lines = ctr->n_lines;
    const uint32_t end = min(ctr->text_len, capacity);   // no store at or behind it
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * HL_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * HL_WAVES;
    for (uint64_t s = (uint64_t)wave * HIT_LINES_SLICE; s < end; s += (uint64_t)n_waves * HIT_LINES_SLICE) {
        const uint32_t s0 = (uint32_t)s, s1 = s + HIT_LINES_SLICE < end ? (uint32_t)(s + HIT_LINES_SLICE) : end;
        // the last line that starts at or in front of the slice: line_off[0] = 0 <= s0 < text_len = line_off[n_lines], strictly ascending
        uint32_t lo = 0, hi = n_lines;
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (line_off[mid] <= s0) lo = mid; else hi = mid; }
        const uint32_t next = line_off[lo + 1];
        if (next >= s1) {   // one line covers the slice: the whole wave copies it
            copy_line(data, data_len, text, src[lo], line_off[lo], next, s0, s1, lane, 64u);
            continue;
        }
        // several lines: one per group of HL_GROUP lanes at a time
        for (uint32_t k = lo + lane / HL_GROUP; k < n_lines; k += 64u / HL_GROUP) {
            const uint32_t o0 = line_off[k];
            if (o0 >= s1) break;
            copy_line(data, data_len, text, src[k], o0, line_off[k + 1], s0, s1, lane % HL_GROUP, HL_GROUP);
        }
    }
}

}  // namespace

uint32_t hit_line_words(uint64_t n_bits) { return (uint32_t)((n_bits + 31) / 32); }
uint32_t hit_line_chunks(uint32_t n) { return std::max<uint32_t>(1u, (uint32_t)(((uint64_t)n + HIT_LINES_SCAN_CHUNK - 1) / HIT_LINES_SCAN_CHUNK)); }

hipError_t hit_lines_mark_rank(const LineRec* fin_lines, uint32_t n_fin, const LineRec* c4_lines, uint32_t n_c4, uint32_t* bitmap, uint64_t n_bits,
                               uint32_t* chunk_sums, uint32_t* word_prefix, HitLineCounters* ctr, hipStream_t stream) {
    if (n_bits > 0xFFFFFFFFull || (uint64_t)n_fin + n_c4 > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t n = n_fin + n_c4, words = hit_line_words(n_bits), chunks = hit_line_chunks(words);
    if (n) hipLaunchKernelGGL(k_hl_mark, dim3((n + HL_THREADS - 1) / HL_THREADS), dim3(HL_THREADS), 0, stream, fin_lines, n_fin, c4_lines, n, bitmap, (uint32_t)n_bits);
    const PopcOf val{bitmap};
    hipLaunchKernelGGL(k_hl_chunk_sum<PopcOf>, dim3(chunks), dim3(HL_THREADS), 0, stream, val, words, (const uint32_t*)nullptr, chunk_sums);
    hipLaunchKernelGGL(k_hl_scan<PopcOf>, dim3(chunks), dim3(HL_THREADS), 0, stream, val, words, (const uint32_t*)nullptr, (const uint32_t*)chunk_sums, word_prefix,
                       &ctr->n_lines);
    return hipGetLastError();
}

hipError_t hit_lines_offsets(const LineRec* fin_lines, uint32_t n_fin, const LineRec* c4_lines, uint32_t n_c4, const uint32_t* bitmap, uint64_t n_bits,
                             const uint32_t* word_prefix, uint32_t* src, uint32_t* len, uint32_t* line_no, uint32_t* line_of, uint32_t* chunk_sums,
                             uint32_t* line_off, HitLineCounters* ctr, hipStream_t stream) {
    if (n_bits > 0xFFFFFFFFull || (uint64_t)n_fin + n_c4 > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t n = n_fin + n_c4, chunks = hit_line_chunks(n);
    if (n) hipLaunchKernelGGL(k_hl_lengths, dim3((n + HL_THREADS - 1) / HL_THREADS), dim3(HL_THREADS), 0, stream, fin_lines, n_fin, c4_lines, n, bitmap, (uint32_t)n_bits,
                              word_prefix, src, len, line_no, line_of);
    const ValueOf val{len};
    hipLaunchKernelGGL(k_hl_chunk_sum<ValueOf>, dim3(chunks), dim3(HL_THREADS), 0, stream, val, n, (const uint32_t*)&ctr->n_lines, chunk_sums);
    hipLaunchKernelGGL(k_hl_scan<ValueOf>, dim3(chunks), dim3(HL_THREADS), 0, stream, val, n, (const uint32_t*)&ctr->n_lines, (const uint32_t*)chunk_sums, line_off,
                       &ctr->text_len);
    return hipGetLastError();
}

hipError_t hit_lines_copy(const uint8_t* data, uint32_t data_len, const HitLineCounters* ctr, const uint32_t* src, const uint32_t* line_off, uint8_t* text,
                          uint32_t capacity, int n_cu, hipStream_t stream) {
    if (capacity == 0) return hipSuccess;   // nothing may be stored; the demand is counted by hit_lines_offsets
    const uint64_t slices = ((uint64_t)capacity + HIT_LINES_SLICE - 1) / HIT_LINES_SLICE;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((slices + HL_WAVES - 1) / HL_WAVES, (uint64_t)std::max(n_cu, 1) * 8u);
    hipLaunchKernelGGL(k_hl_copy, dim3(grid), dim3(HL_THREADS), 0, stream, data, data_len, ctr, src, line_off, text, capacity);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
void HitLines::resolve(const HitBatch& b, const LineRec* fin_lines, const LineRec* c4_lines, uint64_t n_newlines, bool to_host, int n_cu, bool profile,
                       hipStream_t stream) {
    auto grown = [](size_t n) { return n + n / 4 + 1024; };
    const uint32_t n = b.n_fin + b.n_c4;   // records of one fetch stay far below 2^32 (their arrays are indexed with 32 bits)
    const uint64_t n_bits = n_newlines + 1;   // line numbers run from 0 to the '\n' count
    const uint32_t words = hit_line_words(n_bits);
    if (bitmap_.n < words || !word_prefix_.p) { bitmap_.alloc(grown(words)); word_prefix_.alloc(bitmap_.n + 1); }
    const size_t chunks = std::max(hit_line_chunks(words), hit_line_chunks(n));
    if (chunks_.n < chunks) chunks_.alloc(chunks + 64);
    if (src_.n < n || !line_off_.p) {
        const size_t want = grown(n);
        src_.alloc(want); len_.alloc(want); line_no_.alloc(want); line_of_.alloc(want); line_off_.alloc(want + 1);
    }
    if (!ctr_.p) ctr_.alloc(1);
    // the first block of a scanner: 256 bytes per record (a web-server log has lines of ~180); afterwards what the scans before left
    if (!text_.n && n) text_.alloc(std::min<size_t>((size_t)b.len + 1, (size_t)n * 256 + 4096));
    const size_t head = sizeof(HitLineCounters), want = head + (to_host ? ((size_t)3 * n + 1) * 4 : 0);
    pinned_.ensure(want, want / 4 + (1 << 12));
    timed_ = profile; to_host_ = to_host;
    data_ = b.data; data_len_ = b.len; n_fin_ = b.n_fin; n_c4_ = b.n_c4; n_cu_ = n_cu; stream_ = stream;
    if (profile) {
        for (Event& e : ev_) e.create();
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    MXY_HIP(hipMemsetAsync(ctr_.p, 0, sizeof(HitLineCounters), stream));
    if (n) {
        MXY_HIP(hipMemsetAsync(bitmap_.p, 0, (size_t)words * 4, stream));
        MXY_HIP(hit_lines_mark_rank(fin_lines, b.n_fin, c4_lines, b.n_c4, bitmap_.p, n_bits, chunks_.p, word_prefix_.p, ctr_.p, stream));
        MXY_HIP(hit_lines_offsets(fin_lines, b.n_fin, c4_lines, b.n_c4, bitmap_.p, n_bits, word_prefix_.p, src_.p, len_.p, line_no_.p, line_of_.p, chunks_.p,
                                  line_off_.p, ctr_.p, stream));
    } else MXY_HIP(hipMemsetAsync(line_off_.p, 0, 4, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[1], stream));
    if (n) MXY_HIP(hit_lines_copy(b.data, b.len, ctr_.p, src_.p, line_off_.p, text_.p, (uint32_t)std::min<size_t>(text_.n, 0xFFFFFFFFu), n_cu, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[2], stream));
    uint8_t* pb = pinned_.p;
    MXY_HIP(hipMemcpyAsync(pb, ctr_.p, sizeof(HitLineCounters), hipMemcpyDeviceToHost, stream));
    if (to_host) {
        // bounded by the record count, which the host knows: line_off (n + 1), line_no (n), line_of (n); the entries behind n_lines are
        // not meaningful
        MXY_HIP(hipMemcpyAsync(pb + head, line_off_.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, stream));
        if (n) {
            MXY_HIP(hipMemcpyAsync(pb + head + ((size_t)n + 1) * 4, line_no_.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
            MXY_HIP(hipMemcpyAsync(pb + head + ((size_t)2 * n + 1) * 4, line_of_.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        }
    }
}

HitLinesView HitLines::finish() {
    const HitLineCounters c = *reinterpret_cast<const HitLineCounters*>(pinned_.p);
    const uint32_t n = n_fin_ + n_c4_;
    if (timed_) MXY_HIP(hipEventElapsedTime(&ms_[0], ev_[0], ev_[1]));
    bool queued = false;
    if (c.text_len > text_.n) {
        // the block was too small: the demand is exact (counted past the capacity), so one regrow settles it, and only the copy runs again
        text_.alloc((size_t)c.text_len + c.text_len / 4 + 4096);
        if (timed_) MXY_HIP(hipEventRecord(ev_[1], stream_));
        MXY_HIP(hit_lines_copy(data_, data_len_, ctr_.p, src_.p, line_off_.p, text_.p, (uint32_t)std::min<size_t>(text_.n, 0xFFFFFFFFu), n_cu_, stream_));
        if (timed_) MXY_HIP(hipEventRecord(ev_[2], stream_));
        queued = true;
    }
    HitLinesView v;
    v.n_lines = c.n_lines; v.text_len = c.text_len;
    copied_ = 0;
    const bool fetch_text = to_host_ && c.text_len;
    if (fetch_text) {
        pinned_text_.ensure(c.text_len, c.text_len / 4 + (1 << 16));
        if (timed_) MXY_HIP(hipEventRecord(ev_[3], stream_));
        MXY_HIP(hipMemcpyAsync(pinned_text_.p, text_.p, c.text_len, hipMemcpyDeviceToHost, stream_));
        if (timed_) MXY_HIP(hipEventRecord(ev_[4], stream_));
        copied_ = c.text_len;
        queued = true;
    }
    if (queued) MXY_HIP(hipStreamSynchronize(stream_));
    if (timed_) {
        MXY_HIP(hipEventElapsedTime(&ms_[1], ev_[1], ev_[2]));
        ms_[2] = 0;
        if (fetch_text) MXY_HIP(hipEventElapsedTime(&ms_[2], ev_[3], ev_[4]));
    }
    if (to_host_) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(pinned_.p + sizeof(HitLineCounters));
        v.text = fetch_text ? pinned_text_.p : nullptr;
        v.line_off = w;
        v.line_no = n ? w + n + 1 : nullptr;
        v.line_of_fin = n_fin_ ? w + 2 * (size_t)n + 1 : nullptr;
        v.line_of_c4 = n_c4_ ? w + 2 * (size_t)n + 1 + n_fin_ : nullptr;
    } else {
        v.text = c.text_len ? text_.p : nullptr;
        v.line_off = line_off_.p;
        v.line_no = n ? line_no_.p : nullptr;
        v.line_of_fin = n_fin_ ? line_of_.p : nullptr;
        v.line_of_c4 = n_c4_ ? line_of_.p + n_fin_ : nullptr;
    }
    return v;
}

}  // namespace mxy
