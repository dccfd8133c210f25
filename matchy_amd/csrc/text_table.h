// A device-resident table of distinct byte strings that lives across batches (text_table.hip): an open-addressing table of 32-byte
// slots (linear probing, at most half full) beside a pool that holds the text of every entry, so that a later batch, whose log is
// another buffer, can compare against it. The distinct-text set (distinct.h) and the hit tally (tally.h) each own one and differ in
// the key, the claim word and the fourth slot word only.
//
// Three parts: the layout the host and the kernels share (plain functions that tests/cpp/test_text_table_layout.cpp runs on the
// host), the TextTable class that owns the device memory and grows it, and the device templates of the claim and the publish pass,
// which distinct.hip and tally.hip instantiate with their key policy.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>

#include "hashes.h"
#include "hip_owners.h"
#include "scan_types.h"

namespace mxy {

// One slot, 32 bytes (one sector). `state` is the only word more than one lane writes with a compare-and-swap inside a launch:
//   the owner's empty word          free (~0 in the distinct set, 0 in the tally: a table is cleared with 0xFF or zero bytes)
//   a claim word (bit 63 clear)     claimed in the batch that is running by a record of that batch
//   bit 63 set, not the empty word  published: the text is in the pool, `hash` and `text` are valid and never change again (until a reset)
struct TextSlot {
    unsigned long long state;
    unsigned long long hash;   // masked hash the slot was placed with (kept for the rehash and as a filter in front of the byte compare)
    unsigned long long text;   // text_word(): pool offset and length
    unsigned long long aux;    // the owner's: unused in the distinct set, the count in the tally
};
static_assert(sizeof(TextSlot) == 32, "one slot per 32-byte sector");

constexpr unsigned long long TEXT_PUBLISHED = 1ull << 63;
constexpr uint32_t TEXT_NO_SLOT = 0xFFFFFFFFu;
MXY_HD bool text_is_published(unsigned long long state, unsigned long long empty) { return (state >> 63) != 0 && state != empty; }

// MATCHY_AMD_*_HASH_BITS (tests): only that many low bits of the hash are used; 64 and more = all, 0 = every text collides
MXY_HD unsigned long long text_hash_mask(uint32_t bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }
// home slot of a (masked) hash in a table of `slots` (a power of two) entries: the high half is folded in, the low bits alone
// would place the hex hashes of a log by their last digits
MXY_HD uint32_t text_home(unsigned long long hash, uint32_t slot_mask) { return (uint32_t)(hash ^ (hash >> 32)) & slot_mask; }

// pool offset (40 bits, a multiple of TEXT_POOL_ALIGN) and text length (24 bits, the record's length field)
constexpr uint32_t TEXT_POOL_ALIGN = 8;
MXY_HD unsigned long long text_word(unsigned long long pool_off, uint32_t len) { return (pool_off << 24) | (len & 0xFFFFFFu); }
MXY_HD unsigned long long text_word_off(unsigned long long w) { return w >> 24; }
MXY_HD uint32_t text_word_len(unsigned long long w) { return (uint32_t)(w & 0xFFFFFFu); }
MXY_HD unsigned long long text_pool_bytes(uint32_t len) { return ((unsigned long long)len + TEXT_POOL_ALIGN - 1) & ~(unsigned long long)(TEXT_POOL_ALIGN - 1); }

// Slots a table needs so that it is at most half full with `entries` texts: a power of two, at least `floor_slots`.
MXY_HD unsigned long long text_slots_for(unsigned long long entries, unsigned long long floor_slots) {
    unsigned long long s = 16;
    while (s < floor_slots || s < 2 * entries) s <<= 1;
    return s;
}

// The counters, each group in a 128-byte line of its own like ScanCounters: the first lives as long as the table, the second is
// cleared per batch. The distinct set leaves the counting fields unused.
struct TextCounters {
    alignas(128) unsigned long long pool_used;   // bytes of the pool handed out (may pass the capacity: demand of the publish pass)
    alignas(128) unsigned long long n_counted;   // tally: records of the running batch that found a slot (one add per wave)
    uint32_t n_new;                              // slots published in the running batch (one add per wave)
    uint32_t n_pending;                          // winners the publish pass could not store (pool full)
    uint32_t error;                              // bit 0: no free slot on a probe run, bit 1: the same in the rehash (miscounts: the host keeps the table half empty)
    uint32_t n_direct;                           // tally: counts that went past the LDS aggregator straight to the global word
    uint32_t n_export;                           // tally: entries k_tally_export appended
};

// what the kernels of one batch see of the table
struct TextTableView {
    TextSlot* slots;
    uint32_t slot_mask;
    uint8_t* pool;
    unsigned long long pool_cap;
    unsigned long long hash_mask;
    uint32_t* slot_of;       // per record of the running batch: its slot, or TEXT_NO_SLOT
    uint32_t slot_of_cap;
    TextCounters* ctr;
};

// What differs between the owners on the host side: the words of their error texts, their environment variables, their empty word.
struct TextTableOwner {
    const char* who;          // "distinct set" / "hit tally": the prefix of every error text
    const char* entries;      // "texts" / "values"
    const char* reset_call;   // the C call that clears the poisoned state
    const char* full_reason;  // why a full table is a miscount
    const char* env_prefix;   // MATCHY_AMD_DISTINCT_ / MATCHY_AMD_TALLY_ in front of SLOTS, POOL_BYTES, HASH_BITS (tests only)
    unsigned long long empty; // all bytes equal: ~0 or 0
    uint32_t rehash_grid_cap;
};

// Owns the slots, the pool, the counters and the per-batch slot_of array of one table. Not thread-safe. Every method throws
// mxy::HipError. A batch runs as check(), start_batch(), reserve(), open(), the owner's claim launch, publish(), close(); a throw
// between open() and close() leaves claimed slots behind, and check() refuses work until reset().
class TextTable {
public:
    explicit TextTable(const TextTableOwner& owner);
    void reset();                                   // empties the table, keeps the allocations
    void check() const;
    void start_batch(hipStream_t stream);           // the counters exist and their per-batch line is zero
    // Everything that can fail for lack of memory: a table that stays at most half full with `entries` texts, the pool, slot_of for
    // `n_items` records. A failed allocation leaves the table as it was. Returns the number of rehash launches (0 or 1).
    uint32_t reserve(uint64_t entries, size_t n_items, hipStream_t stream);
    TextTableView view() const;
    TextTableView open();                           // view() of a batch that begins: the table counts as inconsistent until close()
    // The publish pass until every winner is stored: `launch` (the owner's kernel, launch check and events) again behind every pool
    // regrow; `view` follows the pool. Ends with the counters in host memory and `stream` synchronised. Returns the number of regrows.
    uint32_t publish(const std::function<void()>& launch, TextTableView& view, hipStream_t stream);
    void close();                                   // the batch is in: takes pool_used and n_new from the counters
    void fetch_counters(hipStream_t stream);        // device -> host, synchronises
    const TextCounters& host_counters() const { return *ctr_host_.p; }
    uint64_t count() const { return count_; }       // entries since creation or the last reset

private:
    void ensure_table(uint64_t entries, hipStream_t stream, uint32_t& rehashes);
    void grow_pool(unsigned long long want, hipStream_t stream);
    const TextTableOwner own_;
    DevBuf<TextSlot> slots_;
    DevBuf<uint8_t> pool_;
    DevBuf<TextCounters> ctr_;
    PinnedBuf<TextCounters> ctr_host_;   // created with ctr_, behind it
    DevBuf<uint32_t> slot_of_;
    uint64_t count_ = 0;
    unsigned long long pool_used_ = 0;   // TextCounters::pool_used behind the last batch
    uint64_t init_slots_, init_pool_;
    uint32_t hash_bits_;
    bool poisoned_ = false;
};

// ------------------------------------------------------------------------------------------------ device: claim and publish
#if defined(__HIPCC__)

__device__ __forceinline__ unsigned long long d_slot_state(const unsigned long long* w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// n bytes at x and y, neither aligned: 8 at a time while 8 are left, then one by one (nothing past n is read)
__device__ __forceinline__ bool d_bytes_equal(const uint8_t* x, const uint8_t* y, uint32_t n) {
    uint32_t o = 0;
    for (; o + 8 <= n; o += 8) {
        unsigned long long a, b;
        __builtin_memcpy(&a, x + o, 8);
        __builtin_memcpy(&b, y + o, 8);
        if (a != b) return false;
    }
    for (; o < n; ++o) if (x[o] != y[o]) return false;
    return true;
}

// A key policy K describes one record of the batch as a key of the table:
//   static constexpr unsigned long long EMPTY     the owner's empty word
//   const uint8_t* text; uint32_t len;            its bytes, inside the batch
//   hash(mask)                                    the masked hash that places it
//   claim_word() / published_word()               what it writes into `state`
//   same_key(published state)                     whatever of the key is in the state word (the tally's type); the bytes are compared here
//   holder_is_me(claim word read from a slot)     does the record of this batch that holds the slot have my key (its bytes are in the same log)
//   join(state pointer, claim word read)          on joining a claimed slot (the distinct set's atomicMin; nothing in the tally)
enum class Probe { Claimed, Joined, Published, Full };

// Walks the probe run of `k` and says how it ended; `slot` is set unless the table was full (a miscount: the host keeps it half empty).
// Different keys never share a slot, whatever their hashes, so there is no retry round. Within one launch a published slot is one of an
// earlier batch: its words and its pool bytes are final.
template <class K>
__device__ __forceinline__ Probe d_text_probe(const TextTableView& t, const K& k, unsigned long long h, uint32_t& slot) {
    const unsigned long long mine = k.claim_word();
    uint32_t i = text_home(h, t.slot_mask);
    for (uint32_t probes = 0; probes <= t.slot_mask; ++probes, i = (i + 1) & t.slot_mask) {
        TextSlot* s = &t.slots[i];
        unsigned long long o = d_slot_state(&s->state);
        if (o == K::EMPTY) {
            o = atomicCAS(&s->state, K::EMPTY, mine);
            if (o == K::EMPTY) { slot = i; return Probe::Claimed; }
        }
        if ((o >> 63) != 0) {
            if (!k.same_key(o) || s->hash != h) continue;
            const unsigned long long tw = s->text, off = text_word_off(tw);
            if (text_word_len(tw) == k.len && off + k.len <= t.pool_cap && d_bytes_equal(t.pool + off, k.text, k.len)) { slot = i; return Probe::Published; }
            continue;
        }
        if (k.holder_is_me(o)) {
            k.join(&s->state, o);
            slot = i;
            return Probe::Joined;
        }
    }
    return Probe::Full;
}

// One turn of the publish pass for a wave. EVERY lane of the wave calls this on every turn: the reservation is wave-wide. A lane with
// `win` still holds `slot` with its own claim word: the winners of the wave reserve pool space with one atomic (inclusive prefix of
// their padded lengths), copy their text, fill in hash and text word (`aux` stays the owner's) and store the published word last. A winner that finds the pool
// full stays claimed and is counted in n_pending. n_new and n_pending are bumped once per wave. Returns whether this lane stored, and
// in `rank` its place among the entries published in this batch (from the n_new add).
// Nobody reads hash / text / pool bytes before the next launch; the lanes of this launch only compare `state` with their own claim word.
template <class K>
__device__ __forceinline__ bool d_text_publish(const TextTableView& t, bool win, uint32_t slot, const K& k, uint32_t lane, uint32_t& rank) {
    rank = 0;
    const unsigned long long winners = __ballot(win);
    if (winners == 0) return false;
    const uint32_t bytes = win ? (uint32_t)text_pool_bytes(k.len) : 0u;
    uint32_t incl = bytes;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    const uint32_t total = __shfl(incl, 63);
    unsigned long long wave_off = 0;
    if (lane == 0 && total) wave_off = atomicAdd(&t.ctr->pool_used, (unsigned long long)total);
    const uint32_t off_lo = __shfl((uint32_t)wave_off, 0), off_hi = __shfl((uint32_t)(wave_off >> 32), 0);
    const unsigned long long off = (((unsigned long long)off_hi << 32) | off_lo) + (incl - bytes);
    const bool stored = win && off + bytes <= t.pool_cap;
    if (stored) {
        uint8_t* dst = t.pool + off;   // 8-byte aligned; the padding bytes behind the text are never read
        uint32_t o = 0;
        for (; o + 8 <= k.len; o += 8) {
            unsigned long long v;
            __builtin_memcpy(&v, k.text + o, 8);
            *reinterpret_cast<unsigned long long*>(dst + o) = v;
        }
        for (; o < k.len; ++o) dst[o] = k.text[o];
        TextSlot* s = &t.slots[slot];
        s->hash = k.hash(t.hash_mask);
        s->text = text_word(off, k.len);
        __hip_atomic_store(&s->state, k.published_word(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long done = __ballot(stored);
    uint32_t new_base = 0;
    if (lane == 0) {
        if (done) new_base = atomicAdd(&t.ctr->n_new, (uint32_t)__popcll(done));
        if (winners & ~done) atomicAdd(&t.ctr->n_pending, (uint32_t)__popcll(winners & ~done));
    }
    rank = __shfl(new_base, 0) + (uint32_t)__popcll(done & ((1ull << lane) - 1ull));
    return stored;
}

#endif  // __HIPCC__

}  // namespace mxy
