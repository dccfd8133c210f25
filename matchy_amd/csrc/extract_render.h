// Extracted candidates as text (extract_render.hip): the candidates of an extraction scan, put into the order of `matchy extract` and
// written as its json / csv / text output on the device. Launch wrappers, the constants the host sizes its buffers with and the tests
// read, and the class that drives the pass for a scanner. The rules of order and text are extract_render_core.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hip_owners.h"
#include "scan_types.h"

namespace mxy {

// A candidate of at most XR_SHORT_MAX text bytes is one lane's work; a longer one goes onto the long list, and a wave measures it and
// later writes it, in strides of 64 bytes.
constexpr uint32_t XR_SHORT_MAX = 512;
// entries one workgroup of the prefix sum over the record lengths covers
constexpr uint32_t XR_SCAN_CHUNK = 2048;
// entries of the candidate lists one workgroup of the key step takes (one add to the pair counter each)
constexpr uint32_t XR_KEY_TILE = 2048;
// MATCHY_AMD_EXTRACT_TEXT_*: REFUSED — the launch was larger than the key holds (xrender::MAX_LEN bytes, 2^32 list entries); nothing ran.
// MISCOUNT — the lists held another number of real entries than the caller said; the block is not valid.
constexpr uint32_t XR_OK = 0, XR_REFUSED = 1, XR_MISCOUNT = 2;

// Counters, each group in a 128-byte line of its own. n_pairs counts the real entries of the lists (past the capacity of the pair
// arrays), n_long the long list, demand the bytes of all records (past the capacity of the block: the work-list contract).
struct alignas(128) XrPairCounter { uint32_t n_pairs; };
struct alignas(128) XrLongCounter { uint32_t n_long; };
struct alignas(128) XrDemand { uint64_t demand; uint32_t status; };
struct alignas(128) XrTypeCounter { uint32_t n; };
struct XrCounters { XrPairCounter pairs; XrLongCounter longs; XrDemand out; XrTypeCounter by_type[IT_COUNT]; };

// What the pass reads, in device memory: the two candidate lists of a one-slice extraction scan (or one list of survivors of the
// distinct set), padding entries (len_type 0xFFFFFFFF) among them, and the `len` bytes they point into (16-byte aligned).
struct XrInput {
    const uint8_t* data = nullptr;
    uint32_t len = 0;
    const Candidate* list_a = nullptr;
    uint32_t n_a = 0;
    const Candidate* list_b = nullptr;
    uint32_t n_b = 0;
    uint32_t n_real = 0;     // real entries of both lists, as the producer counted them: the capacity of the pair arrays
    uint32_t format = 0;     // xrender::FORMAT_*
};

// The arrays of the pass. line_counts: line_tiles(len); line_chunks: line_chunks(..); line_prefix: line_tiles(len) + 1. keys / vals:
// 2 * n_real (the two halves of the sort); sort_temp: sort_hits_temp_bytes(n_real). rec_len: n_real; rec_off: n_real + 1; chunk_sums:
// xr_chunks(n_real); long_list: n_real. ctr: zeroed by the caller in front of extract_render_order.
struct XrWork {
    uint32_t* line_counts;
    uint32_t* line_chunks;
    uint32_t* line_prefix;
    unsigned long long* keys;
    uint32_t* vals;
    void* sort_temp;
    size_t sort_temp_bytes;
    const uint32_t* sort_half;   // xr_sort_half(sort_temp): the half of keys / vals the sort leaves the pairs in
    uint64_t* rec_len;
    uint64_t* rec_off;
    uint64_t* chunk_sums;
    uint32_t* long_list;
    XrCounters* ctr;
};

const uint32_t* xr_sort_half(const void* sort_temp);
size_t sort_hits_temp_bytes(uint32_t n);   // sort_hits.hip: bytes of sort_temp for n pairs
uint32_t xr_chunks(uint32_t n);   // workgroups of the prefix sum over n records (at least one)
// Step 1 + 2: '\n' counts per tile and their prefix, one (key, list index) pair per real entry, the records per type, and the pairs
// sorted by key. hipErrorInvalidValue for a launch the key does not hold (the driver refuses it before).
hipError_t extract_render_order(const XrInput& in, const XrWork& w, int n_cu, hipStream_t stream);
// Step 3: the length of every sorted record and their exclusive prefix: rec_off[0 .. n], ctr->out.demand = rec_off[n]; ctr->out.status.
hipError_t extract_render_measure(const XrInput& in, const XrWork& w, int n_cu, hipStream_t stream);
// Step 4: text[rec_off[i] .. rec_off[i + 1]) = record i, for the bytes in front of min(demand, capacity) and no others. `text` is
// 16-byte aligned. No load reaches data + len.
hipError_t extract_render_write(const XrInput& in, const XrWork& w, uint8_t* text, uint64_t capacity, int n_cu, hipStream_t stream);

// What a fetch with the pass armed hands out. The text of the pieces of one scan_host lie end to end in one pinned block.
struct ExtractTextView {
    bool armed = false;
    const uint8_t* text = nullptr;   // this fetch's records inside the joined block (null: none)
    uint64_t len = 0;
    uint32_t status = XR_OK;
    uint64_t n_records = 0;
    uint64_t by_type[IT_COUNT] = {0};
};

// The pass of a scanner (Scanner::set_extract_text): owns its buffers, grown on demand and reused between scans. Runs once per fetch of
// an extraction scan, over the candidate lists where they lie. The block follows the work-list contract: a block that was too small is
// regrown and the write step alone is repeated. Not thread-safe, like the scanner. Throws mxy::HipError.
class ExtractRender {
public:
    // a new joined block begins (Scanner::scan_host, in front of its pieces)
    void begin() { joined_len_ = 0; }
    // Queues keys, sort, measure and write on `stream`.
    void resolve(const XrInput& in, int n_cu, hipStream_t stream);
    // In place of resolve() for a launch the key does not hold: finish() reports XR_REFUSED.
    void refuse() { refused_ = true; }
    // Behind the wait for `stream`: reads the demand, regrows the block if it was too small and runs the write step alone once more,
    // and copies the block behind the blocks of this joined block so far.
    ExtractTextView finish();
    const uint8_t* joined() const { return joined_len_ ? pinned_text_.p : nullptr; }
    uint64_t joined_len() const { return joined_len_; }
    // device milliseconds of keys + sort, measure, write and the copy of the block of the last finish()
    void timing(float out_ms[4]) const { for (int k = 0; k < 4; ++k) out_ms[k] = ms_[k]; }
    // allocations of the pass's buffers since it was made (a scan like the one before makes none)
    uint64_t allocations() const { return allocations_; }

private:
    XrWork work() const;
    template <class Buf> void grow(Buf& b, size_t want, size_t room);
    DevBuf<uint32_t> line_counts_, line_chunks_, line_prefix_, vals_, long_list_;
    DevBuf<unsigned long long> keys_;
    DevBuf<uint8_t> sort_tmp_, text_;
    DevBuf<uint64_t> rec_len_, rec_off_, chunks_;
    DevBuf<XrCounters> ctr_;
    PinnedBuf<XrCounters> pinned_ctr_;
    PinnedBuf<uint8_t> pinned_text_;
    uint64_t joined_len_ = 0, allocations_ = 0;
    Event ev_[6];
    float ms_[4] = {0, 0, 0, 0};
    // of the resolve() in flight
    XrInput in_{};
    bool refused_ = false, queued_ = false;
    int n_cu_ = 1;
    hipStream_t stream_ = nullptr;
};

}  // namespace mxy
