// Line context of hit records (line_index.hip): launch wrappers and the constants the host sizes its buffers with.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_owners.h"

namespace mxy {

// Bytes per tile of the '\n' count array: one 16-byte load of every lane of a wave. The array costs 4 bytes per tile (0.4 % of the
// batch); a hit's walk over the bytes of its own tile in front of it costs half a tile on average, which is what a larger tile makes
// dearer.
constexpr uint32_t LINE_TILE = 1024;
// Tiles one workgroup of the prefix sum covers (2 MiB of log).
constexpr uint32_t LINE_SCAN_CHUNK = 2048;
constexpr uint32_t LINE_SET_EMPTY = 0xFFFFFFFFu;   // free slot of the distinct-line set (line numbers stay below 2^31)

// 0x80 in every byte of x that is '\n' (exact: no carry crosses a byte): the SWAR test of the '\n' counts, here and in segments.hip
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t nl_bytes(uint32_t x) {
    const uint32_t v = x ^ 0x0A0A0A0Au;
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}
#endif

// One record per hit, bit-identical to matchy_scan_line_t (include/matchy_amd.h).
struct LineRec { uint32_t line, line_start, line_end, reserved; };

// The distinct-line counter of a scan in a 128-byte line of its own.
struct alignas(128) LineCounters { uint32_t distinct; };

uint32_t line_tiles(uint32_t len);
uint32_t line_chunks(uint32_t n_tiles);
// '\n' counts per tile and their exclusive prefix (counts: line_tiles(len) entries, chunk_sums: line_chunks(..), prefix: line_tiles(len) + 1).
// after_count: recorded behind the streaming count kernel when not null (timing).
hipError_t line_index_build(const uint8_t* data, uint32_t len, uint32_t* counts, uint32_t* chunk_sums, uint32_t* prefix, int n_cu, hipStream_t stream,
                            hipEvent_t after_count);
// The prefix step of line_index_build alone (k_line_chunk_sum, k_line_scan), for other per-tile figures (utf16.hip): prefix[t] = sum of
// counts[0 .. t), t = 0 .. n_tiles; n_tiles > 0, chunk_sums: line_chunks(n_tiles) entries.
hipError_t tile_prefix_build(const uint32_t* counts, uint32_t n_tiles, uint32_t* chunk_sums, uint32_t* prefix, hipStream_t stream);
// out[i] for record i of `recs` (n records of `stride` = 16 or 8 bytes that begin with the start offset). set != nullptr: the line numbers
// also go into that set (set_slots: a power of two, at least twice the records of all calls that share it, filled with LINE_SET_EMPTY) and
// *n_distinct grows by the number of lines that were not in it yet.
hipError_t line_index_resolve(const uint8_t* data, uint32_t len, const uint32_t* prefix, const void* recs, uint32_t stride, uint32_t n, LineRec* out,
                              uint32_t* set, uint32_t set_slots, uint32_t* n_distinct, hipStream_t stream);

// The final records of one fetch where they lie in device memory, in the order the caller gets them: `fin` 16-byte records, `c4` 8-byte
// compact records (n_c4 == 0: none), both beginning with the start offset into the `len` bytes at `data`.
struct HitBatch {
    const uint8_t* data;
    uint32_t len;
    const void* fin;
    uint32_t n_fin;
    const void* c4;
    uint32_t n_c4;
};

// Line context of a scanner (Scanner::set_line_context, ScanRequest::lines): owns the buffers of the pass, grown on demand and reused
// between scans. Runs once per fetch, behind the regrow loop — a rescan never counts the batch twice — and behind the sort. Every
// array is written again for exactly the records of that fetch. Not thread-safe, like the scanner. Throws mxy::HipError.
class LineContext {
public:
    // Queues the whole pass on `stream`. to_host: the line records come back into pinned memory like the hit records; otherwise they
    // stay on the device (device_lines) and only the distinct-line count crosses the bus. profile: the pass is timed with events.
    void resolve(const HitBatch& b, bool to_host, int n_cu, bool profile, hipStream_t stream);
    // Behind the wait for `stream`. The arrays are BORROWED from the pinned block (null without to_host or without records) and valid
    // until the next resolve().
    struct Result { uint64_t lines_with_matches = 0; const LineRec* fin_lines = nullptr; const LineRec* c4_lines = nullptr; };
    Result finish();
    // milliseconds of the streaming count kernel, of the prefix sum, and of resolve + distinct set of the last profiled resolve()
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }
    const LineRec* device_lines() const { return recs_.p; }
    const LineRec* device_c4_lines() const { return c4_.p; }
    // What the segment pass of the same fetch reads, meaningful only for the fetch in which resolve() ran: the exclusive '\n' prefix
    // over the tiles, and the distinct-line set with the slots that resolve() used (0: it had no records).
    const uint32_t* prefix() const { return prefix_.p; }
    const uint32_t* set() const { return set_.p; }
    uint32_t set_slots() const { return set_slots_; }

private:
    // '\n' counts per tile, sums per chunk of tiles, exclusive prefix; one line record per final / compact record; the distinct-line
    // set and its counter; the pinned block the counter and (behind it) the line records come back in
    DevBuf<uint32_t> counts_, chunks_, prefix_, set_;
    DevBuf<LineRec> recs_, c4_;
    DevBuf<LineCounters> ctr_;
    PinnedBuf<uint8_t> pinned_;
    Event ev_[4];            // created by the first profiled resolve()
    float ms_[3] = {0, 0, 0};
    uint32_t set_slots_ = 0;
    bool timed_ = false;     // the last resolve() recorded the events
    Result pending_;         // lines_with_matches is filled in by finish()
};

}  // namespace mxy
