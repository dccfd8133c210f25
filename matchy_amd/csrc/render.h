// Rendered records (render.hip): the final records of a fetch as NDJSON text, written on the device. Launch wrappers, the constants
// the host sizes its buffers with and the tests read, and what host and kernels share. The rules of the text are render_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "hip_owners.h"
#include "line_index.h"

namespace mxy {

// ---- bounded serial work. A record is classified from sizes that are known before any of its bytes is read: the length of the hit,
// the length of its line (only where "input_line" is printed) and its id count.
// SHORT: at most RENDER_SHORT_MAX source bytes (hit + line) and at most RENDER_SHORT_IDS ids: one lane measures and writes it.
// LONG: every other record. Whole waves work on it, and each of its two escaped fields is cut into pieces of RENDER_PIECE source bytes
// (the last one shorter; a field of zero bytes has no piece) which are measured and written by one wave each.
constexpr uint32_t RENDER_SHORT_MAX = 512;
constexpr uint32_t RENDER_SHORT_IDS = 8;
constexpr uint32_t RENDER_PIECE = 16384;
// a record of few source bytes whose text (its payloads, that is) exceeds this is LONG as well: a lane never writes more
constexpr uint32_t RENDER_SHORT_TEXT = 8192;
// the payload array of one record ("data":[...]) may take this much text; more ends the pass with RENDER_TOO_LARGE
constexpr uint64_t RENDER_PAYLOAD_ARRAY_MAX = 16ull << 20;
// entries one workgroup of the prefix sum over the record lengths covers
constexpr uint32_t RENDER_SCAN_CHUNK = 2048;
constexpr uint32_t RENDER_OK = 0, RENDER_TOO_LARGE = 1;   // MATCHY_RENDER_OK / MATCHY_RENDER_TOO_LARGE

__host__ __device__ inline uint32_t render_pieces(uint32_t field_len) { return (uint32_t)(((uint64_t)field_len + RENDER_PIECE - 1) / RENDER_PIECE); }
uint32_t render_chunks(uint32_t n);   // workgroups of the prefix sum over n records (at least one)

// ---- payload table: data offset -> JSON text in the pool. Open addressing, a power of two of slots, at most half full; filled by
// the host, read by the kernels. n_slots == 0: an empty table (every lookup misses).
constexpr uint32_t RENDER_KEY_EMPTY = 0xFFFFFFFFu;
struct PayloadSlot { uint32_t key, off, len, reserved; };
struct PayloadTable { const PayloadSlot* slots; uint32_t n_slots; const uint8_t* pool; };
// where the probe sequence of a key begins (linear probing, wrapping); the same rule places the keys of the per-scan miss set
__host__ __device__ inline uint32_t payload_slot(uint32_t key, uint32_t n_slots) {
    const uint32_t h = key * 0x9E3779B1u;
    return (h ^ (h >> 15)) & (n_slots - 1u);
}

// ---- counters, each group in a 128-byte line of its own.
// demand: bytes of all records; it counts past the capacity of the block (the work-list contract). n_pieces is the demand of the
// piece arrays and counts past their capacity; a measure that ran short of piece slots (pieces_short != 0) has no valid demand and is
// repeated with larger arrays.
struct alignas(128) RenderCounters { uint64_t demand, n_pieces; uint32_t status, n_short, n_long, pieces_short; };
// the miss list: distinct data offsets the table did not hold. Counts past the capacity of the list and never writes past it.
struct alignas(128) RenderMissCounter { uint32_t misses; };

struct RenderSource { uint32_t off, len; };   // the escaped source (with its quotes) in the source text
struct RenderLong { uint32_t rec, piece_base, np_line, np_hit; };   // a long record and its slots in the piece arrays

// Everything the pass reads, in device memory. Records in the caller's order: b.fin (16-byte records), then b.c4 (compact IPv4).
struct RenderInput {
    HitBatch b;
    const int64_t* data_offsets = nullptr;     // pattern results: data offset per id (negative: the id has no data)
    uint32_t n_data_offsets = 0;
    uint32_t flags = 0;                        // MATCHY_RENDER_*
    const LineRec* fin_lines = nullptr;        // with line flags: one per record of b.fin / b.c4
    const LineRec* c4_lines = nullptr;
    uint32_t n_segments = 0;                   // 0: one source and one line base (entry 0 of the tables below)
    const uint32_t* seg_of_fin = nullptr;      // n_segments > 0: segment index per record
    const uint32_t* seg_of_c4 = nullptr;
    const uint32_t* seg_line_base = nullptr;   // n_segments > 0 with line flags: '\n' bytes in front of each segment
    const RenderSource* sources = nullptr;     // max(n_segments, 1) entries
    const uint8_t* source_text = nullptr;
    const uint64_t* line_bases = nullptr;      // max(n_segments, 1) entries
};

// The arrays of the pass. rec_len: n records; rec_off: n + 1; chunk_sums: render_chunks(n); long_list: n entries (a list of records
// never outgrows the records); piece_len / piece_off: piece_cap entries; miss_set: miss_set_slots (a power of two, or 0) entries
// filled with RENDER_KEY_EMPTY; miss_list: miss_cap entries.
struct RenderWork {
    uint64_t* rec_len;
    uint64_t* rec_off;
    uint64_t* chunk_sums;
    RenderLong* long_list;
    uint32_t* piece_len;
    uint64_t* piece_off;
    uint32_t piece_cap;
    uint32_t* miss_set;
    uint32_t miss_set_slots;
    uint32_t* miss_list;
    uint32_t miss_cap;
    uint32_t long_hint;         // long records of the scan before (0: none): sizes the grids of the kernels that serve the long list
    RenderCounters* ctr;        // zeroed by the caller in front of render_measure
    RenderMissCounter* miss;    // zeroed by the caller in front of render_measure
};

// Step 1 + 2: the length of every record (short records by one lane, long ones by pieces and waves), the misses of the payload
// table, and the exclusive prefix of the lengths: rec_off[0 .. n], ctr->demand = rec_off[n]. A record whose payload is missing is
// measured with a payload of zero bytes; the demand is exact when the pass reports no miss. max_bytes: a demand above it sets
// ctr->status = RENDER_TOO_LARGE.
hipError_t render_measure(const RenderInput& in, const PayloadTable& table, const RenderWork& w, uint64_t max_bytes, int n_cu, hipStream_t stream);
// Step 3: text[rec_off[i] .. rec_off[i + 1]) = record i, for the bytes in front of min(demand, capacity) and no others. Reads ctr,
// rec_off, the long list and the piece offsets render_measure left, on the device. `text` is 16-byte aligned. No load reaches b.data + b.len.
hipError_t render_write(const RenderInput& in, const PayloadTable& table, const RenderWork& w, uint8_t* text, uint64_t capacity, int n_cu, hipStream_t stream);

// The payload texts of a renderer: data offset -> JSON text, on the host and as the table + pool the kernels read. Lives across
// batches. The host fills it (add), upload() publishes what was added. Bounded: beyond max_entries() it is emptied by its owner.
class PayloadTexts {
public:
    PayloadTexts();
    bool has(uint32_t data_off) const { return find(data_off) != RENDER_KEY_EMPTY; }
    void add(uint32_t data_off, const std::string& json);   // the offset must not be in the table
    void clear();
    void upload(hipStream_t stream);   // waits for the copies: the host vectors may change afterwards
    size_t entries() const { return entries_; }
    uint32_t rehashes() const { return rehashes_; }         // growths of the slot array since the table was made
    uint32_t pool_regrows() const { return pool_regrows_; } // growths of the device pool
    size_t max_entries() const { return max_entries_; }   // MATCHY_AMD_RENDER_PAYLOADS, default 2^20 (the bound of the host renderer's cache)
    PayloadTable view() const { return PayloadTable{slots_dev_.p, (uint32_t)slots_dev_.n, pool_dev_.p}; }   // what upload() last published

private:
    uint32_t find(uint32_t data_off) const;   // slot index, or RENDER_KEY_EMPTY
    void place(const PayloadSlot& s);
    std::vector<PayloadSlot> slots_;   // a power of two, at most half full
    std::vector<uint8_t> pool_;
    size_t entries_ = 0, max_entries_;
    size_t first_slots_, pool_cap_;    // MATCHY_AMD_RENDER_PAYLOADS_SLOTS (64) / _POOL_BYTES (64 KiB): where table and device pool start (tests)
    uint32_t rehashes_ = 0, pool_regrows_ = 0;
    DevBuf<PayloadSlot> slots_dev_;
    DevBuf<uint8_t> pool_dev_;
};

// What a scan with the renderer armed hands out: the block (pinned host memory, or device memory for a fetch that leaves its records
// on the device), BORROWED until the scanner's next scan.
struct RenderView { bool armed = false; const uint8_t* text = nullptr; uint64_t len = 0; uint32_t status = RENDER_OK; };

// What arms a scan (Scanner::set_render): the sources arrive escaped, with their quotes.
struct RenderParams {
    uint32_t flags = 0;
    bool per_segment = false;            // one source and one line base per segment of the scan
    std::vector<std::string> sources;    // one entry, or one per segment
    std::vector<uint64_t> line_bases;    // parallel to sources
};

// The renderer of a scanner: owns the buffers of the pass and the payload texts, grown on demand and reused between scans. Runs once
// per fetch behind the line pass and the segment pass, whose device arrays it reads. The block follows the work-list contract, like
// the block of hit lines. Not thread-safe, like the scanner. Throws mxy::HipError.
class NdjsonRender {
public:
    // payload JSON of a data offset ("null" where the value does not decode): payload_json (engine.h), which the host renderer uses too
    using PayloadFn = void (*)(const void* ctx, uint32_t data_off, std::string& json);
    // The tables of the scan go to the device on `stream`, in front of its kernels.
    void arm(const RenderParams& p, hipStream_t stream);
    // Queues measure, offsets and write on `stream`. `in` carries the device arrays of the fetch; its sources, line bases and flags
    // are filled in here. to_host: finish() fetches the block into pinned memory; otherwise it stays on the device.
    void resolve(RenderInput in, bool to_host, int n_cu, bool profile, hipStream_t stream);
    // Behind the wait for `stream`: renders and uploads the payloads the table missed and repeats the pass until none is missing,
    // regrows the block if it was too small and runs the write step alone once more, and (to_host) copies `demand` bytes.
    RenderView finish(PayloadFn payload, const void* ctx);
    // milliseconds of measure + offsets, of the write step (the last run of each), and of the block's device-to-host copy
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }
    // of the last finish(): repeats of the pass, payloads rendered, bytes copied to the host
    struct Events { uint32_t rounds = 0, payloads_added = 0, rehashes = 0, pool_regrows = 0; uint64_t misses = 0, copied = 0; };
    const Events& last_events() const { return events_; }
    uint32_t flags() const { return params_.flags; }
    bool per_segment() const { return params_.per_segment; }
    size_t n_sources() const { return params_.sources.size(); }

private:
    void queue_round(bool measure);
    RenderWork work() const;
    PayloadTexts texts_;
    RenderParams params_;
    std::vector<RenderSource> source_table_;   // what arm() uploads: alive until the next arm()
    std::string source_text_;
    uint32_t long_hint_ = 0;
    DevBuf<RenderSource> sources_dev_;
    DevBuf<uint8_t> source_text_dev_;
    DevBuf<uint64_t> line_bases_dev_;
    DevBuf<uint64_t> rec_len_, rec_off_, chunks_, piece_off_;
    DevBuf<RenderLong> long_list_;
    DevBuf<uint32_t> piece_len_, miss_set_, miss_list_;
    DevBuf<uint8_t> text_;
    DevBuf<uint8_t> ctr_;               // RenderCounters, then RenderMissCounter
    PinnedBuf<uint8_t> pinned_;         // the two counter blocks as read back
    PinnedBuf<uint8_t> pinned_text_;
    Event ev_[5];
    float ms_[3] = {0, 0, 0};
    Events events_;
    uint64_t max_bytes_ = 0;
    // of the resolve() in flight
    RenderInput in_{};
    bool to_host_ = false, timed_ = false;
    int n_cu_ = 1;
    hipStream_t stream_ = nullptr;
};

}  // namespace mxy
