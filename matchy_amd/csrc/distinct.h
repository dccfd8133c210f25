// Device-resident set of the distinct candidate texts an extractor handle has returned (distinct.hip): `extract --unique`.
//
// The first part of this header is the layout the host and the kernels share (slot words, order key, hash masking): plain functions
// that tests/cpp/test_distinct_layout.cpp runs on the host. The DistinctSet class behind it drives the kernels.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hashes.h"
#include "scan_types.h"

namespace mxy {

// One slot of the open-addressing table, 32 bytes (one sector). `order` is the only word more than one lane writes inside a launch:
//   DISTINCT_EMPTY                  free
//   an order key (bit 63 clear)     claimed in the batch that is running: the least key of the candidates with this text so far
//   DISTINCT_PUBLISHED              the text is in the pool: `hash` and `text` are valid and never change again (until a reset)
struct DistinctSlot {
    unsigned long long order;
    unsigned long long hash;   // masked hash the slot was placed with (kept for the rehash and as a filter in front of the byte compare)
    unsigned long long text;   // distinct_text_word(): pool offset and length
    unsigned long long reserved;
};
static_assert(sizeof(DistinctSlot) == 32, "one slot per 32-byte sector");

constexpr unsigned long long DISTINCT_EMPTY = ~0ull;
constexpr unsigned long long DISTINCT_PUBLISHED = 1ull << 63;
constexpr uint32_t DISTINCT_NO_SLOT = 0xFFFFFFFFu;

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

// MATCHY_AMD_DISTINCT_HASH_BITS (tests): only that many low bits of the hash are used; 64 and more = all, 0 = every text collides
MXY_HD unsigned long long distinct_hash_mask(uint32_t bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }
// home slot of a (masked) hash in a table of `slots` (a power of two) entries: the high half is folded in, the low bits alone
// would place the hex hashes of a log by their last digits
MXY_HD uint32_t distinct_home(unsigned long long hash, uint32_t slot_mask) { return (uint32_t)(hash ^ (hash >> 32)) & slot_mask; }

// pool offset (40 bits, a multiple of DISTINCT_POOL_ALIGN) and text length (24 bits, the candidate record's length field)
constexpr uint32_t DISTINCT_POOL_ALIGN = 8;
MXY_HD unsigned long long distinct_text_word(unsigned long long pool_off, uint32_t len) { return (pool_off << 24) | (len & 0xFFFFFFu); }
MXY_HD unsigned long long distinct_text_off(unsigned long long w) { return w >> 24; }
MXY_HD uint32_t distinct_text_len(unsigned long long w) { return (uint32_t)(w & 0xFFFFFFu); }
MXY_HD unsigned long long distinct_pool_bytes(uint32_t len) { return ((unsigned long long)len + DISTINCT_POOL_ALIGN - 1) & ~(unsigned long long)(DISTINCT_POOL_ALIGN - 1); }

// Slots a table needs so that it is at most half full with `entries` texts: a power of two, at least `floor_slots`.
MXY_HD unsigned long long distinct_slots_for(unsigned long long entries, unsigned long long floor_slots) {
    unsigned long long s = 16;
    while (s < floor_slots || s < 2 * entries) s <<= 1;
    return s;
}

// The counters of the set, each in a 128-byte line of its own like ScanCounters: both are bumped once per wave.
struct DistinctCounters {
    alignas(128) unsigned long long pool_used;   // bytes of the pool handed out (may pass the capacity: demand of the publish pass)
    alignas(128) uint32_t n_out;                 // survivors of the running batch
    uint32_t n_pending;                          // winners the publish pass could not store (pool full)
    uint32_t error;                              // bit 0: no free slot on a probe run, bit 1: the same in the rehash (miscounts: the host keeps the table half empty)
};

// Owned by one extractor handle (Scanner::set_unique); lives across chunks and pieces. Not thread-safe, like the scanner.
// Every method throws mxy::HipError; after a throw from filter() the set refuses work until reset().
class DistinctSet {
public:
    DistinctSet();
    ~DistinctSet();
    DistinctSet(const DistinctSet&) = delete;
    DistinctSet& operator=(const DistinctSet&) = delete;
    // Keeps, of the candidates of one batch (two lists, padding entries have len_type 0xFFFFFFFF; `cand_true` real ones), those whose
    // text log[start, start + len) is not in the set yet — per text the one with the least (start, type rank) — adds their texts, and
    // copies exactly them to `out`. Synchronises `stream`.
    void filter(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                std::vector<Candidate>& out, hipStream_t stream);
    void reset();                                  // empties the set, keeps the allocations
    uint64_t count() const { return count_; }      // distinct texts since creation or the last reset
    // HIP-event milliseconds of the dedup kernels of the last filter() (growth included), when set_profile(true)
    void set_profile(bool on) { profile_ = on; }
    float last_ms() const { return last_ms_; }

private:
    void ensure_table(uint64_t entries, hipStream_t stream);
    void grow_pool(unsigned long long want, hipStream_t stream);
    DistinctSlot* slots_ = nullptr;
    uint64_t n_slots_ = 0;
    uint8_t* pool_ = nullptr;
    unsigned long long pool_cap_ = 0;
    DistinctCounters* ctr_ = nullptr;        // device
    DistinctCounters* ctr_host_ = nullptr;   // pinned
    uint32_t* slot_of_ = nullptr;            // per candidate of the running batch: its slot, or DISTINCT_NO_SLOT
    size_t slot_of_n_ = 0;
    Candidate* out_dev_ = nullptr;
    size_t out_n_ = 0;
    uint64_t count_ = 0;
    unsigned long long pool_used_ = 0;       // DistinctCounters::pool_used behind the last batch
    uint64_t init_slots_, init_pool_;
    uint32_t hash_bits_;
    bool poisoned_ = false, profile_ = false;
    hipEvent_t ev_[2] = {nullptr, nullptr};
    float last_ms_ = 0;
};

}  // namespace mxy
