// Device-resident set of the distinct candidate texts an extractor handle has returned (distinct.hip): `extract --unique`.
//
// The table itself is a TextTable (text_table.h). The first part of this header is what is the set's own of the layout the host and the
// kernels share (order key, type rank): plain functions that tests/cpp/test_distinct_layout.cpp runs on the host. The DistinctSet class
// behind it drives the kernels.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "scan_types.h"
#include "text_table.h"

namespace mxy {

// The `state` word of a slot (text_table.h), the only word more than one lane writes inside a launch:
//   DISTINCT_EMPTY                  free
//   an order key (bit 63 clear)     claimed in the batch that is running: the least key of the candidates with this text so far
//   DISTINCT_PUBLISHED              the text is in the pool
constexpr unsigned long long DISTINCT_EMPTY = ~0ull;
constexpr unsigned long long DISTINCT_PUBLISHED = TEXT_PUBLISHED;

// Order key of a candidate inside one batch: (start, type rank, index in the batch's candidate lists). The least key of a text is the
// candidate that stays; the index makes keys unique and leads back to the candidate's bytes. Bit 63 stays clear.
constexpr uint32_t DISTINCT_START_BITS = 30, DISTINCT_RANK_BITS = 4, DISTINCT_INDEX_BITS = 29;
static_assert(DISTINCT_START_BITS + DISTINCT_RANK_BITS + DISTINCT_INDEX_BITS == 63, "bit 63 tells keys from the other states");
constexpr uint32_t DISTINCT_MAX_LEN = 1u << DISTINCT_START_BITS;        // batches of at most this many bytes (starts below it)
constexpr uint32_t DISTINCT_MAX_INDEX = 1u << DISTINCT_INDEX_BITS;      // candidate list entries of one batch, padding included

// chunk-path extractor order, as d_type_rank (sort_hits.hip) and type_rank (capi.cpp)
MXY_HD uint32_t distinct_type_rank(uint32_t t) {
    switch (t) {
        case IT_IPV6: return 0; case IT_IPV4: return 1; case IT_EMAIL: return 2; case IT_DOMAIN: return 3;
        case IT_MD5: case IT_SHA1: case IT_SHA256: case IT_SHA384: case IT_SHA512: return 4;
        case IT_BITCOIN: return 5; case IT_ETHEREUM: return 6; case IT_MONERO: return 7;
    }
    return 8;
}
MXY_HD unsigned long long distinct_order_key(uint32_t start, uint32_t item_type, uint32_t index) {
    return ((unsigned long long)start << (DISTINCT_RANK_BITS + DISTINCT_INDEX_BITS)) |
           ((unsigned long long)distinct_type_rank(item_type) << DISTINCT_INDEX_BITS) | (unsigned long long)index;
}
MXY_HD uint32_t distinct_key_index(unsigned long long key) { return (uint32_t)(key & (DISTINCT_MAX_INDEX - 1u)); }
MXY_HD bool distinct_is_key(unsigned long long order) { return (order >> 63) == 0; }

// Owned by one extractor handle (Scanner::set_unique); lives across chunks and pieces. Not thread-safe, like the scanner.
// Every method throws mxy::HipError; after a throw from filter() the set refuses work until reset().
class DistinctSet {
public:
    DistinctSet();
    // Keeps, of the candidates of one batch (two lists, padding entries have len_type 0xFFFFFFFF; `cand_true` real ones), those whose
    // text log[start, start + len) is not in the set yet — per text the one with the least (start, type rank) — adds their texts, and
    // copies exactly them to `out`. Synchronises `stream`.
    void filter(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                std::vector<Candidate>& out, hipStream_t stream);
    // The same, with the survivors left in device memory: returns their number; survivors() holds them (no padding entries among them)
    // until the next filter call.
    uint32_t filter_device(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                           hipStream_t stream);
    const Candidate* survivors() const { return out_dev_.p; }
    void reset();                                  // empties the set, keeps the allocations
    uint64_t count() const { return table_.count(); }   // distinct texts since creation or the last reset
    // HIP-event milliseconds of the dedup kernels of the last filter() (growth included), when set_profile(true)
    void set_profile(bool on) { profile_ = on; }
    float last_ms() const { return last_ms_; }

private:
    uint32_t run(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                 hipStream_t stream, bool& open);
    TextTable table_;
    DevBuf<Candidate> out_dev_;
    bool profile_ = false;
    Event ev_[2];   // created by the first profiled filter()
    float last_ms_ = 0;
};

}  // namespace mxy
