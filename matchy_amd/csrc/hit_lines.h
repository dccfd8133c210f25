// Hit lines (hit_lines.hip): the distinct lines that carry a hit, packed into one block on the device. Launch wrappers, the constants
// the host sizes its buffers with, and the pass of a scanner.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_owners.h"
#include "line_index.h"

namespace mxy {

// Bytes of the block one wave of the copy kernel owns: it searches the offsets once and then writes these bytes and no others.
constexpr uint32_t HIT_LINES_SLICE = 4096;
// Entries one workgroup of the two prefix sums covers: words of the line bitmap (32 lines each) in the rank step, lines in the
// offset step.
constexpr uint32_t HIT_LINES_SCAN_CHUNK = 2048;

// The two figures of a gather that only the device knows, in a 128-byte line of their own. text_len is the DEMAND: it counts past the
// capacity of the block (the work-list contract), and it fits 32 bits because the block is at most one byte longer than the batch —
// the lines are disjoint ranges of the batch, every terminated one contains the '\n' the block ends it with, and only an unterminated
// last line gets a byte the batch does not have: text_len <= len + 1 < 2^31 + 1. Offsets into the block are 32-bit for that reason.
struct alignas(128) HitLineCounters { uint32_t n_lines, text_len; };

uint32_t hit_line_words(uint64_t n_bits);    // 32-bit words of a bitmap of n_bits lines
uint32_t hit_line_chunks(uint32_t n);        // workgroups of a prefix sum over n entries (at least one)

// Step 1 + 2. One bit per line of the batch that holds a record (bitmap: hit_line_words(n_bits) words, cleared by the caller; a line
// number at or above n_bits is ignored), then the exclusive popcount prefix over the words (word_prefix: words + 1 entries; chunk_sums:
// hit_line_chunks(words)); the total, the number of distinct lines, also goes to ctr->n_lines.
hipError_t hit_lines_mark_rank(const LineRec* fin_lines, uint32_t n_fin, const LineRec* c4_lines, uint32_t n_c4, uint32_t* bitmap, uint64_t n_bits,
                               uint32_t* chunk_sums, uint32_t* word_prefix, HitLineCounters* ctr, hipStream_t stream);
// Step 3 + 4. rank(line) = word_prefix[line >> 5] + popc(bitmap word below the line's bit). Every record stores line_of[i] = rank (fin
// records first, then the compact ones) and the three values of its line at [rank] — all records of a line carry the same start and
// end, so they store the same values and no winner has to be chosen. Then line_off[0 .. n_lines] = exclusive prefix of len[] (the
// arrays: n_fin + n_c4 entries, line_off one more; chunk_sums: hit_line_chunks(n_fin + n_c4)), and ctr->text_len = line_off[n_lines].
hipError_t hit_lines_offsets(const LineRec* fin_lines, uint32_t n_fin, const LineRec* c4_lines, uint32_t n_c4, const uint32_t* bitmap, uint64_t n_bits,
                             const uint32_t* word_prefix, uint32_t* src, uint32_t* len, uint32_t* line_no, uint32_t* line_of, uint32_t* chunk_sums,
                             uint32_t* line_off, HitLineCounters* ctr, hipStream_t stream);
// Step 5. text[line_off[k] .. line_off[k + 1] - 1) = data[src[k] ..), '\n' at line_off[k + 1] - 1, for the bytes below `capacity` and
// no others. ctr, src and line_off are read on the device. `data` and `text` are 16-byte aligned; no load reaches data + data_len.
hipError_t hit_lines_copy(const uint8_t* data, uint32_t data_len, const HitLineCounters* ctr, const uint32_t* src, const uint32_t* line_off, uint8_t* text,
                          uint32_t capacity, int n_cu, hipStream_t stream);

// What a fetch with hit lines hands out. line_of_fin / line_of_c4 are parallel to the final / compact records of the fetch.
struct HitLinesView {
    const uint8_t* text = nullptr;
    uint64_t text_len = 0;
    uint32_t n_lines = 0;
    const uint32_t* line_off = nullptr;   // n_lines + 1 entries
    const uint32_t* line_no = nullptr;    // n_lines
    const uint32_t* line_of_fin = nullptr;
    const uint32_t* line_of_c4 = nullptr;
};

// Hit lines of a scanner (Scanner::set_hit_lines, ScanRequest::hit_lines): owns the buffers of the pass, grown on demand and reused
// between scans. Runs once per fetch behind LineContext::resolve, whose device arrays it reads. The block follows the work-list
// contract: the copy kernel is queued against the capacity the previous scans left, every store sits behind that capacity, the demand
// is read behind the fetch's wait, and a block that was too small is grown and only the copy kernel runs again. Not thread-safe, like
// the scanner. Throws mxy::HipError.
class HitLines {
public:
    // Queues steps 1 - 5 on `stream`. n_newlines: '\n' bytes of the batch (line numbers run from 0 to it). to_host: the index arrays
    // come back into pinned memory with this fetch and finish() fetches the block; otherwise everything stays on the device.
    void resolve(const HitBatch& b, const LineRec* fin_lines, const LineRec* c4_lines, uint64_t n_newlines, bool to_host, int n_cu, bool profile, hipStream_t stream);
    // Behind the wait for `stream`: reads the demand, regrows and re-runs the copy kernel if it did not fit, and (to_host) copies
    // text_len bytes of the block and waits once more. The arrays are BORROWED (pinned memory, or device memory without to_host) and
    // valid until the next resolve().
    HitLinesView finish();
    // milliseconds of mark + rank + lengths + offsets, of the copy kernel (the last run of it), and of the block's device-to-host copy
    void timing(float out_ms[3]) const { for (int k = 0; k < 3; ++k) out_ms[k] = ms_[k]; }
    uint64_t last_copied_bytes() const { return copied_; }   // bytes of the block that crossed the bus in the last finish()

private:
    DevBuf<uint32_t> bitmap_, word_prefix_, chunks_, src_, len_, line_no_, line_off_, line_of_;
    DevBuf<uint8_t> text_;
    DevBuf<HitLineCounters> ctr_;
    PinnedBuf<uint8_t> pinned_;        // the counters, then line_off, line_no and line_of of the fetch
    PinnedBuf<uint8_t> pinned_text_;
    Event ev_[5];                      // created by the first profiled resolve()
    float ms_[3] = {0, 0, 0};
    uint64_t copied_ = 0;
    bool timed_ = false, to_host_ = false;
    // of the resolve() in flight
    const uint8_t* data_ = nullptr;
    uint32_t data_len_ = 0, n_fin_ = 0, n_c4_ = 0;
    int n_cu_ = 1;
    hipStream_t stream_ = nullptr;
};

}  // namespace mxy
