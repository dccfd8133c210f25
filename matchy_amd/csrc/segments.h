// Segmented scans (segments.hip): a batch described as a sequence of newline-terminated segments. Launch wrappers and what the host
// and the kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hip_owners.h"
#include "line_index.h"

namespace mxy {

// One entry per segment, bit-identical to matchy_scan_segment_t (include/matchy_amd.h).
struct SegmentRec { uint32_t start, len, hits, line_base, lines, lines_with_matches, reserved[2]; };
static_assert(sizeof(SegmentRec) == 32, "one segment per 32-byte sector");

// In front of the segment table in device memory, so that both come back in one copy. bad: the lowest index of a segment that breaks
// the newline rule (SEG_NONE: none). total_nl: '\n' bytes of the batch (line context only).
struct SegHeader { uint32_t bad, total_nl, reserved[6]; };
static_assert(sizeof(SegHeader) == 32, "keeps the table 32-byte aligned");
constexpr uint32_t SEG_NONE = 0xFFFFFFFFu;

// The sample table of the record pass: every seg_sample_stride(n)-th start, at most SEG_SAMPLES entries (4 KiB of LDS).
constexpr uint32_t SEG_SAMPLES = 1024;
inline uint32_t seg_sample_stride(uint32_t n) { return n ? (n + SEG_SAMPLES - 1) / SEG_SAMPLES : 1u; }
inline uint32_t seg_sample_count(uint32_t n) { const uint32_t st = seg_sample_stride(n); return (n + st - 1) / st; }

// Segment pass. starts: n entries in device memory (host-checked: starts[0] == 0, non-decreasing, all <= len). Writes hdr, table[0, n)
// (hits and lines_with_matches zero), line_base[0, n) and sample[0, seg_sample_count(n)). prefix: the exclusive '\n' prefix over the
// LINE_TILE-byte tiles of the batch (line_index_build), or null without line context (line_base stays 0).
hipError_t segments_build(const uint8_t* data, uint32_t len, const uint32_t* starts, uint32_t n, const uint32_t* prefix, SegHeader* hdr, SegmentRec* table,
                          uint32_t* line_base, uint32_t* sample, hipStream_t stream);
// Record pass. seg_of[i] = the last segment whose start is <= the start of record i (n_recs records of `stride` = 16 or 8 bytes that
// begin with the start offset); table[seg].hits grows by the records of the segment.
hipError_t segments_attribute(const void* recs, uint32_t stride, uint32_t n_recs, uint32_t len, const uint32_t* starts, uint32_t n, const uint32_t* sample,
                              uint32_t* seg_of, SegmentRec* table, hipStream_t stream);
// Lines-with-matches pass over the distinct-line set line_index_resolve left (set_slots slots, LINE_SET_EMPTY = free): every line number
// in it counts for the last segment whose line_base is <= it.
hipError_t segments_count_lines(const uint32_t* set, uint32_t set_slots, const uint32_t* line_base, uint32_t n, SegmentRec* table, hipStream_t stream);

// What the segment pass reads of the line context of the same fetch (LineContext::prefix, set, set_slots); the default is a fetch
// without line context.
struct SegLines {
    const uint32_t* prefix = nullptr;
    const uint32_t* set = nullptr;
    uint32_t set_slots = 0;
};

// Segmented scans of a scanner (Scanner::set_segments): the caller's table from set() to the fetch of the scan it describes, and the
// buffers of the pass, grown on demand and reused between scans. A scan runs as set(), arm(), upload() in front of its kernels,
// resolve() in its fetch and finish() behind the wait. Not thread-safe, like the scanner. Throws mxy::HipError and, for a table that
// breaks its rules, mxy::ParamError.
class SegmentPass {
public:
    // `starts` (copied) describes the buffer of the next lookup scan; n == 0 or null clears a pending table
    void set(const uint32_t* starts, size_t n);
    // Consumes the pending table, whether the scan succeeds or not (none: the scan has no segments), and checks it against the `len`
    // bytes of the scan: starts[0] == 0, non-decreasing, every start <= len.
    void arm(size_t len);
    bool active() const { return active_; }
    bool pending() const { return !pending_.empty(); }   // set() left a table that no scan has armed yet
    void off() { active_ = false; index_base_ = 0; }
    // The armed table goes to the device on `stream`, in front of the scan's kernels: the copy of a pageable vector is staged by the
    // runtime, and behind the scan it would sit on the critical path of the fetch.
    void upload(hipStream_t stream);
    // A scan in pieces: take() hands the armed table out and switches the pass off; arm_piece() arms the segments first..last of that
    // table for the piece that starts at byte `pos` of the whole (starts clamped to the piece and made relative to it), with `first` as
    // the index base of finish()'s error text. OffAtExit switches the pass off when the scan in pieces ends, however it ends.
    std::vector<uint32_t> take();
    void arm_piece(const std::vector<uint32_t>& all, size_t first, size_t last, uint32_t pos);
    struct OffAtExit { SegmentPass* s; ~OffAtExit() { if (s) s->off(); } };
    // Queues the pass on `stream`, behind the line context it builds on, over the records in the order the caller gets them. to_host: the
    // segment indices come back into pinned memory like the hit records; otherwise they stay on the device (device_of_fin) and only header
    // + table cross the bus, in one copy.
    void resolve(const HitBatch& b, const SegLines& lines, bool to_host, bool profile, hipStream_t stream);
    // Behind the wait for `stream`: throws ParamError when a segment breaks the newline rule, fills in the lines of every segment (line
    // context). Everything is BORROWED from the pinned block and valid until the next resolve().
    struct Result { const SegmentRec* segments = nullptr; size_t n_segments = 0; const uint32_t* seg_of_fin = nullptr; const uint32_t* seg_of_c4 = nullptr; };
    Result finish();
    // milliseconds of the segment pass, the record passes and the lines-with-matches pass of the last profiled resolve()
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }
    const uint32_t* device_of_fin() const { return of_fin_.p; }
    const uint32_t* device_of_c4() const { return of_c4_.p; }
    // what the renderer of the same fetch reads: the segments of the scan in flight, and the '\n' count in front of each (line context)
    size_t armed_count() const { return active_ ? starts_.size() : 0; }
    const uint32_t* device_line_base() const { return line_base_.p; }

private:
    std::vector<uint32_t> pending_, starts_;   // the table set() left, and the one of the scan in flight
    bool active_ = false;
    uint32_t index_base_ = 0;                  // a scan in pieces: the caller's index of the first segment of the piece in flight
    // the armed table on the device, line_base per segment, the sample table, one segment index per final / compact record; header +
    // table in one block; the pinned block header, table and (to_host) the indices come back in
    DevBuf<uint32_t> starts_dev_, line_base_, sample_, of_fin_, of_c4_;
    DevBuf<uint8_t> table_;
    PinnedBuf<uint8_t> pinned_;
    Event ev_[4];                              // created by the first profiled resolve()
    float ms_[3] = {0, 0, 0};
    bool timed_ = false, with_lines_ = false;  // of the last resolve()
    Result result_;
};

}  // namespace mxy
