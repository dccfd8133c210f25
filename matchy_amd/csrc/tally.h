// Device-resident tally of the hits of a scanner per distinct matched value (tally.hip): `matchy match --tally`, matchy_scanner_set_tally.
//
// The key of an entry is (item type, matched text): the bytes log[start, start + len) of a final record and the type the extractor gave
// them. The first part of this header is what the host and the kernels share (slot words, record decoding, the type-seeded hash) and the
// host-only ordering / merge logic of the read-out: plain functions that tests/cpp/test_tally_layout.cpp runs on the host. The HitTally
// class behind it drives the kernels. The table itself is a TextTable (text_table.h); distinct.h is here for the type rank of the order.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "distinct.h"

namespace mxy {

// The `state` word of a slot (text_table.h), the only word more than one lane writes with a compare-and-swap inside a launch; the
// slot's `aux` word is the count, which is only ever added to:
//   TALLY_EMPTY (0)                 free: a table is cleared with zero bytes, which also makes every count 0
//   index + 1 (bits 32.. clear)     claimed in the batch that is running by the record with that index; every record that joins has
//                                   the same type and bytes, so it does not matter which one holds the slot
//   TALLY_PUBLISHED | item type     the text is in the pool
constexpr unsigned long long TALLY_EMPTY = 0;
constexpr unsigned long long TALLY_PUBLISHED = TEXT_PUBLISHED;
constexpr uint64_t TALLY_MAX_RECORDS = 0xFFFFFFF0ull;   // records of one batch: index + 1 stays below 2^32

MXY_HD bool tally_is_published(unsigned long long state) { return (state >> 63) != 0; }
MXY_HD uint32_t tally_state_type(unsigned long long state) { return (uint32_t)(state & 0xFFu); }
MXY_HD unsigned long long tally_published(uint32_t item_type) { return TALLY_PUBLISHED | (item_type & 0xFFu); }
MXY_HD unsigned long long tally_claim_word(uint32_t index) { return (unsigned long long)index + 1ull; }
MXY_HD uint32_t tally_claim_index(unsigned long long state) { return (uint32_t)(state - 1ull); }

// text length of a compact IPv4 record (scan_types.h c4_pack: length - 7 in bits 22..25 of the second word)
MXY_HD uint32_t tally_c4_len(uint32_t packed) { return ((packed >> C4_DATA_BITS) & 15u) + 7u; }
// a record is used only when its text lies inside the batch
MXY_HD bool tally_usable(uint32_t start, uint32_t n, uint32_t len) { return start < len && n <= len - start; }
// The item type is part of the key: it seeds the hash (and is compared before the bytes). MATCHY_AMD_TALLY_HASH_BITS masks the result
// (text_hash_mask): 0 bits make every (type, text) collide.
MXY_HD unsigned long long tally_hash(const uint8_t* text, uint32_t n, uint32_t item_type, unsigned long long mask) { return xxh64(text, n, item_type) & mask; }

// One published entry as k_tally_export writes it; `text` is the slot's text word, `slot` leads back to the table.
struct TallyExport {
    unsigned long long count;
    unsigned long long text;
    uint32_t item_type;
    uint32_t slot;
};
static_assert(sizeof(TallyExport) == 24, "three words");
// One text k_tally_gather copies: from the pool (text word) to `dst_off` of the gather buffer.
struct TallyGather { unsigned long long text; unsigned long long dst_off; };

// ------------------------------------------------------------------------------------------------ host: order, selection, merge
struct TallyEntry {
    std::string text;    // raw log bytes
    uint8_t item_type = 0;
    uint64_t count = 0;
};

// The order of a read-out: count descending, then the extractor order of the type, then the text bytewise ascending (a proper prefix
// first). Two entries of one tally never compare equal beyond (rank, text) unless their types share a rank (the hash lengths): the type
// itself breaks that tie, so the order is total.
inline bool tally_entry_less(const TallyEntry& a, const TallyEntry& b) {
    if (a.count != b.count) return a.count > b.count;
    const uint32_t ra = distinct_type_rank(a.item_type), rb = distinct_type_rank(b.item_type);
    if (ra != rb) return ra < rb;
    const size_t n = std::min(a.text.size(), b.text.size());
    const int c = n ? memcmp(a.text.data(), b.text.data(), n) : 0;
    if (c != 0) return c < 0;
    if (a.text.size() != b.text.size()) return a.text.size() < b.text.size();
    return a.item_type < b.item_type;
}
inline void tally_order(std::vector<TallyEntry>& v, size_t limit) {
    std::sort(v.begin(), v.end(), tally_entry_less);
    if (limit && v.size() > limit) v.resize(limit);
}

// Which exported entries a top-`limit` read-out needs the texts of: the order above up to the text is known from the export alone, so
// everything in front of the limit-th entry by (count, rank) is in, and so is the whole group that ties with it (the texts decide inside
// it). limit 0 or limit >= size: all. Returns indices into `ex`.
inline std::vector<uint32_t> tally_select(const std::vector<TallyExport>& ex, size_t limit) {
    std::vector<uint32_t> idx(ex.size());
    for (size_t i = 0; i < ex.size(); ++i) idx[i] = (uint32_t)i;
    if (!limit || limit >= ex.size()) return idx;
    auto key_less = [&](uint32_t a, uint32_t b) {
        if (ex[a].count != ex[b].count) return ex[a].count > ex[b].count;
        return distinct_type_rank(ex[a].item_type) < distinct_type_rank(ex[b].item_type);
    };
    std::nth_element(idx.begin(), idx.begin() + (limit - 1), idx.end(), key_less);
    const uint32_t cut = idx[limit - 1];
    std::vector<uint32_t> out;
    for (uint32_t i : idx) if (!key_less(cut, i)) out.push_back(i);   // in front of the cut entry, or tied with it
    return out;
}

// The read-outs of several workers as one: counts of equal (type, text) add up.
inline std::vector<TallyEntry> tally_merge(const std::vector<std::vector<TallyEntry>>& parts) {
    std::map<std::pair<uint8_t, std::string>, uint64_t> sum;
    for (const auto& p : parts) for (const TallyEntry& e : p) sum[{e.item_type, e.text}] += e.count;
    std::vector<TallyEntry> out;
    out.reserve(sum.size());
    for (const auto& kv : sum) { TallyEntry e; e.item_type = kv.first.first; e.text = kv.first.second; e.count = kv.second; out.push_back(std::move(e)); }
    return out;
}

// Owned by one scanner (Scanner::set_tally); lives across batches and pieces. Not thread-safe, like the scanner.
// Every method throws mxy::HipError; after a throw from add() the tally refuses work until reset().
class HitTally {
public:
    HitTally();
    // Counts the records of one batch whose text log[start, start + len) lies inside it: `final` (16-byte records, all kinds) and `c4`
    // (compact IPv4 records; null / 0 when compact records are not in effect), both in device memory like `log`. Synchronises `stream`.
    void add(const uint8_t* log, uint32_t len, const FinalHit* final, uint32_t n_final, const uint2* c4, uint32_t n_c4, hipStream_t stream);
    void reset();                                      // empties the tally, keeps the allocations
    uint64_t distinct() const { return table_.count(); }   // entries since creation or the last reset
    uint64_t matches() const { return matches_; }      // records counted (the sum of all counts)
    // The first `limit` entries in read-out order (0 = all): the counts of all entries come back, the texts of the chosen ones only.
    void top(size_t limit, std::vector<TallyEntry>& out, hipStream_t stream);
    void export_all(std::vector<TallyEntry>& out, hipStream_t stream) { top(0, out, stream); }
    // HIP-event milliseconds of the last add() (growth included) and of its claim / publish kernels alone, when set_profile(true)
    void set_profile(bool on) { profile_ = on; }
    float last_ms() const { return last_ms_; }
    float last_claim_ms() const { return claim_ms_; }
    float last_publish_ms() const { return publish_ms_; }
    // what the last add() did besides counting (trace line, tests): tables rehashed, pools regrown, counts past the LDS aggregator
    struct Events { uint32_t rehashes = 0, pool_regrows = 0, direct_adds = 0, new_entries = 0; };
    const Events& last_events() const { return events_; }

private:
    TextTable table_;
    uint64_t matches_ = 0;
    bool profile_ = false;
    Event ev_[3];   // created by the first profiled add()
    float last_ms_ = 0, claim_ms_ = 0, publish_ms_ = 0;
    Events events_;
};

}  // namespace mxy
