// Segmented scans, on the GPU: the caller describes a batch as a sequence of newline-terminated segments (the files of a pack), the scan
// runs once as for any batch, and the passes here attribute its records to the segments where they lie:
//   k_seg_build     one lane per segment: the newline rule (the byte in front of the next start of a non-empty segment that is not the
//                   last must be '\n'; the lowest offending index goes into an error word with atomicMin), the segment's entry of the
//                   table, with line context its line_base (prefix of the tile of its start + the '\n' bytes of that tile in front of
//                   it, the SWAR test of line_index.hip), and every stride-th start into the sample table
//   k_seg_records   one lane per record: the last segment whose start is <= the record's start, by an upper bound in two levels — the
//                   sample table in LDS, then the <= stride starts behind the sample in global memory — and the segment's hit count
//   k_seg_lines     line context: one lane per slot of the distinct-line set; an occupied slot counts for the last segment whose
//                   line_base is <= its line number
// The two counting passes count through the workgroup's LDS aggregator (lds_aggregator.h: segment -> count, four leader rounds) — a
// batch whose hits sit in one large segment would otherwise put every wave on one counter line. No lane waits for another, every loop
// has a fixed bound, nothing is stored without a bound test, and no load of log bytes reaches `len`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "lds_aggregator.h"
#include "line_index.h"
#include "segments.h"

namespace mxy {

namespace {

constexpr uint32_t SEG_THREADS = 256;
constexpr uint32_t SEG_ITEMS = 1024;          // records (slots) per workgroup at least, while the grid allows: what one flush of the aggregator covers
constexpr uint32_t SEG_MAX_GRID = 2048;
using SegAgg = LdsAggregator<7, 4, 4>;
constexpr uint32_t SEG_AGG_SLOTS = SegAgg::SLOTS;
static_assert(SegAgg::NO_KEY == SEG_NONE, "no segment has the aggregator's free key");
constexpr uint32_t SEG_WORDS = sizeof(SegmentRec) / 4;   // the counters of neighbouring segments lie this many words apart
// LDS is handed out in 1280-byte granules: sample table + aggregator are four of them, the aggregator alone is padded to one
constexpr uint32_t SEG_LDS_RECORDS = SEG_SAMPLES + 2 * SEG_AGG_SLOTS, SEG_LDS_LINES = 320;
static_assert(SEG_LDS_RECORDS * 4 % 1280 == 0 && SEG_LDS_LINES * 4 % 1280 == 0 && SEG_LDS_LINES >= 2 * SEG_AGG_SLOTS, "whole LDS granules");

// the last index i of [lo, hi) with a[i] <= x, given a[lo] <= x (a is non-decreasing): at most 32 turns
template <class A>
__device__ __forceinline__ uint32_t last_le(A a, uint32_t lo, uint32_t hi, uint32_t x) {
    for (uint32_t turn = 0; turn < 32u && hi - lo > 1u; ++turn) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_build(const uint8_t* __restrict__ data, uint32_t len, const uint32_t* __restrict__ starts, uint32_t n,
                                                           const uint32_t* __restrict__ prefix, uint32_t n_tiles, SegHeader* __restrict__ hdr,
                                                           SegmentRec* __restrict__ table, uint32_t* __restrict__ line_base, uint32_t* __restrict__ sample,
                                                           uint32_t stride) {
    const uint32_t s = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (s == 0) hdr->total_nl = prefix ? prefix[n_tiles] : 0u;
    if (s >= n) return;
    // the host has checked the table; the clamps keep every offset inside the batch whatever it holds
    const uint32_t start = min(starts[s], len);
    const uint32_t end = max(s + 1 < n ? min(starts[s + 1], len) : len, start);
    if (s + 1 < n && end > start && data[end - 1] != (uint8_t)'\n') atomicMin(&hdr->bad, s);
    uint32_t lb = 0;
    if (prefix) {
        const uint32_t tile = start / LINE_TILE;   // <= n_tiles: the prefix array has n_tiles + 1 entries
        uint32_t off = tile * LINE_TILE, cnt = 0;  // `data` is 16-byte aligned and every byte in front of start lies inside the batch
        for (; off + 16u <= start; off += 16u) {   // < LINE_TILE / 16 turns
            const uint4 v = *reinterpret_cast<const uint4*>(data + off);
            cnt += __popc(nl_bytes(v.x)) + __popc(nl_bytes(v.y)) + __popc(nl_bytes(v.z)) + __popc(nl_bytes(v.w));
        }
        for (; off + 4u <= start; off += 4u) cnt += __popc(nl_bytes(*reinterpret_cast<const uint32_t*>(data + off)));
        for (; off < start; ++off) cnt += data[off] == (uint8_t)'\n' ? 1u : 0u;
        lb = prefix[tile] + cnt;
    }
    uint4* row = reinterpret_cast<uint4*>(table + s);
    row[0] = make_uint4(start, end - start, 0u, lb);
    row[1] = make_uint4(0u, 0u, 0u, 0u);
    line_base[s] = lb;
    if (s % stride == 0 && s / stride < SEG_SAMPLES) sample[s / stride] = start;
}

// One count per lane of `counting` for its segment into `field` of the table (&table[0].hits or .lines_with_matches). Every lane of
// the wave calls this: the leader rounds are wave-wide. An add the aggregator has no room for goes to the global word.
__device__ __forceinline__ void d_seg_count(uint32_t* keys, uint32_t* counts, bool valid, uint32_t seg, uint32_t lane, uint32_t* __restrict__ field) {
    const uint32_t direct = SegAgg::count(keys, counts, __ballot(valid), seg, lane);
    if (direct) atomicAdd(&field[(size_t)seg * SEG_WORDS], direct);
}
__device__ __forceinline__ void d_seg_flush(const uint32_t* keys, const uint32_t* counts, uint32_t n, uint32_t* __restrict__ field) {
    SegAgg::flush(keys, counts, SEG_THREADS, [=](uint32_t k, uint32_t c) {
        if (k < n) atomicAdd(&field[(size_t)k * SEG_WORDS], c);
    });
}

// STRIDE: bytes of a record (16: FinalHit, 8: compact IPv4 record); both begin with the start offset. n_samples = seg_sample_count(n) and
// stride = seg_sample_stride(n) as k_seg_build wrote the sample table; hits = &table[0].hits.
template <uint32_t STRIDE>
__global__ __launch_bounds__(SEG_THREADS) void k_seg_records(const uint8_t* __restrict__ recs, uint32_t n_recs, uint32_t len, const uint32_t* __restrict__ starts,
                                                             uint32_t n, const uint32_t* __restrict__ sample, uint32_t n_samples, uint32_t stride,
                                                             uint32_t* __restrict__ seg_of, uint32_t* __restrict__ hits) {
    __shared__ uint32_t lds[SEG_LDS_RECORDS];
    uint32_t* smp = lds;
    uint32_t* keys = lds + SEG_SAMPLES;
    uint32_t* counts = keys + SEG_AGG_SLOTS;
    for (uint32_t e = threadIdx.x; e < n_samples && e < SEG_SAMPLES; e += SEG_THREADS) smp[e] = sample[e];
    SegAgg::clear(keys, counts, SEG_THREADS);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * SEG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * SEG_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the counting is wave-wide
    for (uint32_t base = wave * 64u; base < n_recs; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        const bool valid = idx < n_recs;
        uint32_t seg = 0;
        if (valid) {
            const uint32_t x = min(*reinterpret_cast<const uint32_t*>(recs + (size_t)idx * STRIDE), len);   // a record never starts behind the batch
            const uint32_t j = last_le(smp, 0u, n_samples, x);        // smp[0] = starts[0] = 0 <= x
            const uint32_t lo = j * stride;                           // starts[lo] = smp[j] <= x < smp[j + 1] = starts[lo + stride]
            seg = last_le(starts, lo, min(lo + stride, n), x);        // ties: the last equal start, so an empty segment owns nothing
            seg_of[idx] = seg;
        }
        d_seg_count(keys, counts, valid, seg, lane, hits);
    }
    __syncthreads();
    d_seg_flush(keys, counts, n, hits);
}

// set: the distinct-line set of line_index_resolve; lwm = &table[0].lines_with_matches
__global__ __launch_bounds__(SEG_THREADS) void k_seg_lines(const uint32_t* __restrict__ set, uint32_t set_slots, const uint32_t* __restrict__ line_base, uint32_t n,
                                                           uint32_t* __restrict__ lwm) {
    __shared__ uint32_t lds[SEG_LDS_LINES];
    uint32_t* keys = lds;
    uint32_t* counts = lds + SEG_AGG_SLOTS;
    SegAgg::clear(keys, counts, SEG_THREADS);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * SEG_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * SEG_THREADS) >> 6;
    for (uint32_t base = wave * 64u; base < set_slots; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        const uint32_t line = idx < set_slots ? set[idx] : LINE_SET_EMPTY;
        const bool valid = line != LINE_SET_EMPTY;
        // line_base[0] = 0 <= line. A non-empty segment in front of the last ends in '\n', so equal neighbours are empty segments and
        // an unterminated line can only belong to the last one: the last segment with line_base <= line is the line's segment
        const uint32_t seg = valid ? last_le(line_base, 0u, n, line) : 0u;
        d_seg_count(keys, counts, valid, seg, lane, lwm);
    }
    __syncthreads();
    d_seg_flush(keys, counts, n, lwm);
}

uint32_t grid_for(uint32_t items) { return std::max<uint32_t>(1u, std::min<uint32_t>((items + SEG_ITEMS - 1) / SEG_ITEMS, SEG_MAX_GRID)); }

}  // namespace

hipError_t segments_build(const uint8_t* data, uint32_t len, const uint32_t* starts, uint32_t n, const uint32_t* prefix, SegHeader* hdr, SegmentRec* table,
                          uint32_t* line_base, uint32_t* sample, hipStream_t stream) {
    if (n == 0) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(hdr, 0xFF, sizeof(SegHeader), stream);   // bad = SEG_NONE
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_seg_build, dim3((n + SEG_THREADS - 1) / SEG_THREADS), dim3(SEG_THREADS), 0, stream, data, len, starts, n, prefix, line_tiles(len), hdr, table,
                       line_base, sample, seg_sample_stride(n));
    return hipGetLastError();
}

hipError_t segments_attribute(const void* recs, uint32_t stride, uint32_t n_recs, uint32_t len, const uint32_t* starts, uint32_t n, const uint32_t* sample,
                              uint32_t* seg_of, SegmentRec* table, hipStream_t stream) {
    if (n_recs == 0) return hipSuccess;
    if (n == 0 || (stride != 16 && stride != 8)) return hipErrorInvalidValue;
    if (stride == 16)
        hipLaunchKernelGGL(k_seg_records<16>, dim3(grid_for(n_recs)), dim3(SEG_THREADS), 0, stream, (const uint8_t*)recs, n_recs, len, starts, n, sample,
                           seg_sample_count(n), seg_sample_stride(n), seg_of, &table->hits);
    else
        hipLaunchKernelGGL(k_seg_records<8>, dim3(grid_for(n_recs)), dim3(SEG_THREADS), 0, stream, (const uint8_t*)recs, n_recs, len, starts, n, sample,
                           seg_sample_count(n), seg_sample_stride(n), seg_of, &table->hits);
    return hipGetLastError();
}

hipError_t segments_count_lines(const uint32_t* set, uint32_t set_slots, const uint32_t* line_base, uint32_t n, SegmentRec* table, hipStream_t stream) {
    if (set_slots == 0) return hipSuccess;
    if (n == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_seg_lines, dim3(grid_for(set_slots)), dim3(SEG_THREADS), 0, stream, set, set_slots, line_base, n, &table->lines_with_matches);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ host driver
void SegmentPass::set(const uint32_t* starts, size_t n) {
    if (!starts || !n) { pending_.clear(); return; }
    pending_.assign(starts, starts + n);
}

void SegmentPass::arm(size_t len) {
    off();
    starts_.clear();
    starts_.swap(pending_);
    if (starts_.empty()) return;
    std::string bad;
    if (starts_.size() > 0x7FFFFFFFull) bad = "segments: too many segments";
    else if (starts_[0] != 0) bad = "segments: starts[0] must be 0";
    for (size_t s = 0; bad.empty() && s < starts_.size(); ++s) {
        if (starts_[s] > len) bad = "segments: start of segment " + std::to_string(s) + " lies behind the end of the buffer";
        else if (s && starts_[s] < starts_[s - 1]) bad = "segments: start of segment " + std::to_string(s) + " lies in front of its predecessor's";
    }
    if (!bad.empty()) { starts_.clear(); throw ParamError{bad}; }
    active_ = true;
}

std::vector<uint32_t> SegmentPass::take() {
    std::vector<uint32_t> all;
    if (active_) all.swap(starts_);
    off();
    return all;
}

void SegmentPass::arm_piece(const std::vector<uint32_t>& all, size_t first, size_t last, uint32_t pos) {
    starts_.resize(last - first + 1);
    for (size_t k = 0; k < starts_.size(); ++k) starts_[k] = std::max(all[first + k], pos) - pos;
    active_ = true;
    index_base_ = (uint32_t)first;
}

void SegmentPass::upload(hipStream_t stream) {
    const size_t n = starts_.size();
    if (starts_dev_.n < n) {
        starts_dev_.alloc(n + n / 4 + 1024); line_base_.alloc(starts_dev_.n);
        table_.alloc(sizeof(SegHeader) + starts_dev_.n * sizeof(SegmentRec));
    }
    MXY_HIP(hipMemcpyAsync(starts_dev_.p, starts_.data(), n * 4, hipMemcpyHostToDevice, stream));
}

void SegmentPass::resolve(const HitBatch& b, const SegLines& lines, bool to_host, bool profile, hipStream_t stream) {
    auto grown = [](uint32_t n) { return (size_t)n + n / 4 + 1024; };
    const uint32_t n = (uint32_t)starts_.size();
    const size_t n_recs = (size_t)b.n_fin + b.n_c4;
    if (!sample_.p) sample_.alloc(SEG_SAMPLES);
    if (of_fin_.n < b.n_fin) of_fin_.alloc(grown(b.n_fin));
    if (of_c4_.n < b.n_c4) of_c4_.alloc(grown(b.n_c4));
    const size_t head = sizeof(SegHeader) + (size_t)n * sizeof(SegmentRec), want = head + (to_host ? n_recs * 4 : 0);
    pinned_.ensure(want, want / 4 + (1 << 16));
    timed_ = profile;
    with_lines_ = lines.prefix != nullptr;
    if (profile) {
        for (Event& e : ev_) e.create();
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    SegHeader* hdr = reinterpret_cast<SegHeader*>(table_.p);
    SegmentRec* table = reinterpret_cast<SegmentRec*>(table_.p + sizeof(SegHeader));
    MXY_HIP(segments_build(b.data, b.len, starts_dev_.p, n, lines.prefix, hdr, table, line_base_.p, sample_.p, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[1], stream));
    MXY_HIP(segments_attribute(b.fin, 16, b.n_fin, b.len, starts_dev_.p, n, sample_.p, of_fin_.p, table, stream));
    MXY_HIP(segments_attribute(b.c4, 8, b.n_c4, b.len, starts_dev_.p, n, sample_.p, of_c4_.p, table, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[2], stream));
    if (with_lines_ && lines.set_slots) MXY_HIP(segments_count_lines(lines.set, lines.set_slots, line_base_.p, n, table, stream));
    if (profile) MXY_HIP(hipEventRecord(ev_[3], stream));
    uint8_t* pb = pinned_.p;
    MXY_HIP(hipMemcpyAsync(pb, table_.p, head, hipMemcpyDeviceToHost, stream));
    result_ = Result{};
    if (to_host) {
        if (b.n_fin) MXY_HIP(hipMemcpyAsync(pb + head, of_fin_.p, (size_t)b.n_fin * 4, hipMemcpyDeviceToHost, stream));
        if (b.n_c4) MXY_HIP(hipMemcpyAsync(pb + head + (size_t)b.n_fin * 4, of_c4_.p, (size_t)b.n_c4 * 4, hipMemcpyDeviceToHost, stream));
        result_.seg_of_fin = b.n_fin ? (const uint32_t*)(pb + head) : nullptr;
        result_.seg_of_c4 = b.n_c4 ? (const uint32_t*)(pb + head) + b.n_fin : nullptr;
    }
    result_.segments = reinterpret_cast<const SegmentRec*>(pb + sizeof(SegHeader));
    result_.n_segments = n;
}

// the error word, and the lines of every segment from neighbouring line_base values and the batch's total
SegmentPass::Result SegmentPass::finish() {
    const SegHeader* hdr = reinterpret_cast<const SegHeader*>(pinned_.p);
    SegmentRec* t = reinterpret_cast<SegmentRec*>(pinned_.p + sizeof(SegHeader));
    const size_t n = result_.n_segments;
    if (timed_) for (int k = 0; k < 3; ++k) MXY_HIP(hipEventElapsedTime(&ms_[k], ev_[k], ev_[k + 1]));
    if (hdr->bad != SEG_NONE)
        throw ParamError{"segments: segment " + std::to_string((size_t)hdr->bad + index_base_) + " does not end in a newline (every non-empty segment in front of the last must)"};
    if (with_lines_) for (size_t s = 0; s < n; ++s) t[s].lines = (s + 1 < n ? t[s + 1].line_base : hdr->total_nl) - t[s].line_base;
    return result_;
}

}  // namespace mxy
