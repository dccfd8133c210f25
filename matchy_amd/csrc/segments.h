// Segmented scans (segments.hip): a batch described as a sequence of newline-terminated segments. Launch wrappers and what the host
// and the kernels share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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

}  // namespace mxy
