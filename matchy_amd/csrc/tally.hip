// Hit tally on the GPU (`matchy match --tally`, matchy_scanner_set_tally): how often every distinct matched value hit, kept in device
// memory across batches — an open-addressing table of 32-byte slots {state, hash, text word, count} (linear probing, at most half full)
// beside a pool with the text of every entry — and read out as a top-N list. It is fed from the final records of a scan while the
// batch is still resident, so nothing but counters and the rows of the report ever crosses the bus.
//
// The key is (item type, matched text): an XXH64 of the text seeded with the type picks the home slot; equality is decided by comparing
// the type and then the bytes. The 16-byte records and the compact IPv4 records of a batch form one index space.
//
//   k_tally_claim     one lane per record. It walks the probe run of its key: a published slot (an earlier batch) with the same type,
//                     hash, length and bytes is its entry; a slot claimed in this batch holds the index of a record of this batch,
//                     whose bytes are in the same log — equal type and bytes: the lane joins it; an empty slot is claimed with a
//                     compare-and-swap of the lane's own index. All holders of a slot have identical bytes, so no order key is needed.
//                     The lane then counts: lanes of a wave that found the slot of the wave's first lane add once together; every add
//                     goes through the workgroup's LDS aggregator (slot index -> count), which is flushed with one global atomic per
//                     occupied entry when the workgroup ends: a workgroup covers at least 1024 records, so a million hits on one
//                     address end in about a thousand global atomics (by construction, not by measurement).
//   k_tally_publish   the record whose index is still in its slot stores the text: the winners of a wave reserve pool space with one
//                     atomic, copy their bytes, fill in hash and text word and mark the slot published with the type. The count word
//                     is not touched. A winner that finds the pool full stays claimed and is counted as pending; the host grows the
//                     pool and runs the pass again for exactly those.
//   k_tally_rehash    moves the published slots, with their counts, into a larger table. Between batches only.
//   k_tally_export    the published slots as a dense array {count, text word, type, slot}, one atomic per wave.
//   k_tally_gather    the texts of a host-chosen list of entries into one contiguous buffer (one wave per text).
//
// No lane waits for another: every probe loop is bounded by the table size or by TALLY_AGG_PROBES, and a table that is full against
// expectation sets an error bit.
#include "tally.h"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "engine.h"

namespace mxy {

namespace {

constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_CLAIM_ITEMS = 1024;   // records per workgroup of k_tally_claim at least (while the grid allows): what one flush of the aggregator covers

struct TallyParams {
    const uint8_t* log;
    uint32_t len;
    const FinalHit* recs;      // entries [0, n_recs) of the batch's index space
    uint32_t n_recs;
    const uint2* c4;           // entries [n_recs, n_recs + n_c4)
    uint32_t n_c4;
    TallySlot* slots;
    uint32_t slot_mask;
    uint8_t* pool;
    unsigned long long pool_cap;
    unsigned long long hash_mask;
    uint32_t* slot_of;
    uint32_t slot_of_cap;
    TallyCounters* ctr;
};

struct Rec { uint32_t start, len, type; };
__device__ __forceinline__ Rec d_rec(const TallyParams& p, uint32_t i) {
    Rec r;
    if (i < p.n_recs) {
        const FinalHit h = p.recs[i];
        r.start = h.start; r.len = h.len_type & 0xFFFFFFu; r.type = h.len_type >> 24;
    } else {
        const uint2 c = p.c4[i - p.n_recs];
        r.start = c.x; r.len = tally_c4_len(c.y); r.type = IT_IPV4;
    }
    return r;
}
__device__ __forceinline__ unsigned long long d_state(const unsigned long long* w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// n bytes at x and y, neither aligned: 8 at a time while 8 are left, then one by one (nothing past n is read)
__device__ __forceinline__ bool d_same_bytes(const uint8_t* x, const uint8_t* y, uint32_t n) {
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

// `add` hits for table slot `slot` into the workgroup's aggregator; false when the key found no room within TALLY_AGG_PROBES probes
__device__ __forceinline__ bool d_agg_add(uint32_t* keys, uint32_t* counts, uint32_t slot, uint32_t add) {
    uint32_t h = tally_agg_home(slot);
#pragma unroll
    for (uint32_t t = 0; t < TALLY_AGG_PROBES; ++t, h = (h + 1u) & (TALLY_AGG_SLOTS - 1u)) {
        uint32_t k = keys[h];
        if (k == TALLY_NO_SLOT) k = atomicCAS(&keys[h], TALLY_NO_SLOT, slot);
        if (k == TALLY_NO_SLOT || k == slot) { atomicAdd(&counts[h], add); return true; }
    }
    return false;
}

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_claim(const TallyParams p) {
    __shared__ uint32_t agg_keys[TALLY_AGG_SLOTS];
    __shared__ uint32_t agg_counts[TALLY_AGG_SLOTS];
    for (uint32_t e = threadIdx.x; e < TALLY_AGG_SLOTS; e += TALLY_THREADS) { agg_keys[e] = TALLY_NO_SLOT; agg_counts[e] = 0; }
    __syncthreads();
    const uint32_t n = p.n_recs + p.n_c4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the counting below is wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        uint32_t found = TALLY_NO_SLOT;
        if (idx < n) {
            const Rec r = d_rec(p, idx);
            if (tally_usable(r.start, r.len, p.len)) {
                const uint8_t* text = p.log + r.start;
                const unsigned long long h = tally_hash(text, r.len, r.type, p.hash_mask);
                const unsigned long long mine = tally_claim_word(idx);
                uint32_t i = distinct_home(h, p.slot_mask);
                for (uint32_t probes = 0; probes <= p.slot_mask; ++probes, i = (i + 1) & p.slot_mask) {
                    TallySlot* s = &p.slots[i];
                    unsigned long long o = d_state(&s->state);
                    if (o == TALLY_EMPTY) {
                        o = atomicCAS(&s->state, TALLY_EMPTY, mine);
                        if (o == TALLY_EMPTY) { found = i; break; }
                    }
                    if (tally_is_published(o)) {   // an earlier batch's entry: its words and its pool bytes are final
                        if (tally_state_type(o) != r.type || s->hash != h) continue;
                        const unsigned long long tw = s->text;
                        const unsigned long long off = distinct_text_off(tw);
                        if (distinct_text_len(tw) == r.len && off + r.len <= p.pool_cap && d_same_bytes(p.pool + off, text, r.len)) { found = i; break; }
                        continue;
                    }
                    // claimed in this batch by a record of this batch: the same key joins it, any other walks on
                    const uint32_t hidx = tally_claim_index(o);
                    if (hidx >= n) continue;
                    const Rec holder = d_rec(p, hidx);
                    if (holder.type == r.type && holder.len == r.len && tally_usable(holder.start, holder.len, p.len) &&
                        d_same_bytes(p.log + holder.start, text, r.len)) { found = i; break; }
                }
                if (found == TALLY_NO_SLOT) atomicOr(&p.ctr->error, 1u);   // a full table: the host keeps it half empty, so this is a miscount
            }
            if (idx < p.slot_of_cap) p.slot_of[idx] = found;
        }
        // count: the lanes that share the slot of the wave's first counting lane add once, the others one by one
        const bool counts = found != TALLY_NO_SLOT;
        const unsigned long long counting = __ballot(counts);
        if (counting == 0) continue;
        const uint32_t first = (uint32_t)__ffsll((long long)counting) - 1u;
        const uint32_t lead = __shfl(found, first);
        const unsigned long long same = __ballot(counts && found == lead);
        bool direct = false;
        if (counts) {
            if (found != lead) direct = !d_agg_add(agg_keys, agg_counts, found, 1u);
            else if (lane == first) direct = !d_agg_add(agg_keys, agg_counts, found, (uint32_t)__popcll(same));
            if (direct) atomicAdd(&p.slots[found].count, found != lead ? 1ull : (unsigned long long)__popcll(same));
        }
        const unsigned long long past = __ballot(direct);
        if (lane == first) {
            atomicAdd(&p.ctr->n_counted, (unsigned long long)__popcll(counting));
            if (past) atomicAdd(&p.ctr->n_direct, (uint32_t)__popcll(past));
        }
    }
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < TALLY_AGG_SLOTS; e += TALLY_THREADS) {
        const uint32_t k = agg_keys[e], c = agg_counts[e];
        if (k != TALLY_NO_SLOT && c && k <= p.slot_mask) atomicAdd(&p.slots[k].count, (unsigned long long)c);
    }
}

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_publish(const TallyParams p) {
    const uint32_t n = p.n_recs + p.n_c4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the reservation below is wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        Rec r{0, 0, 0};
        uint32_t slot = TALLY_NO_SLOT;
        bool win = false;
        if (idx < n && idx < p.slot_of_cap) {
            slot = p.slot_of[idx];
            if (slot <= p.slot_mask) {
                r = d_rec(p, idx);
                win = d_state(&p.slots[slot].state) == tally_claim_word(idx) && tally_usable(r.start, r.len, p.len);
            }
        }
        const unsigned long long winners = __ballot(win);
        if (winners == 0) continue;
        // pool space: inclusive prefix of the winners' (padded) lengths over the wave, one atomic for the sum
        const uint32_t bytes = win ? (uint32_t)distinct_pool_bytes(r.len) : 0u;
        uint32_t incl = bytes;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const uint32_t total = __shfl(incl, 63);
        unsigned long long wave_off = 0;
        if (lane == 0 && total) wave_off = atomicAdd(&p.ctr->pool_used, (unsigned long long)total);
        const uint32_t off_lo = __shfl((uint32_t)wave_off, 0), off_hi = __shfl((uint32_t)(wave_off >> 32), 0);
        const unsigned long long off = (((unsigned long long)off_hi << 32) | off_lo) + (incl - bytes);
        const bool stored = win && off + bytes <= p.pool_cap;
        if (stored) {
            const uint8_t* text = p.log + r.start;
            uint8_t* dst = p.pool + off;   // 8-byte aligned; the padding bytes behind the text are never read
            uint32_t o = 0;
            for (; o + 8 <= r.len; o += 8) {
                unsigned long long v;
                __builtin_memcpy(&v, text + o, 8);
                *reinterpret_cast<unsigned long long*>(dst + o) = v;
            }
            for (; o < r.len; ++o) dst[o] = text[o];
            TallySlot* s = &p.slots[slot];
            s->hash = tally_hash(text, r.len, r.type, p.hash_mask);
            s->text = distinct_text_word(off, r.len);
            // `count` was added to by the claim pass and stays. Nobody reads hash / text / pool bytes before the next launch; the lanes of
            // this launch only compare `state` with their own claim word
            __hip_atomic_store(&s->state, tally_published(r.type), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long done = __ballot(stored);
        if (lane == 0) {
            if (done) atomicAdd(&p.ctr->n_new, (uint32_t)__popcll(done));
            if (winners & ~done) atomicAdd(&p.ctr->n_pending, (uint32_t)__popcll(winners & ~done));
        }
    }
}

// published slots of the old table, counts included, into the new one (zero-filled); the keys are distinct, so nothing is compared
__global__ __launch_bounds__(TALLY_THREADS) void k_tally_rehash(const TallySlot* old_slots, uint32_t n_old, TallySlot* slots, uint32_t slot_mask, TallyCounters* ctr) {
    for (uint32_t k = blockIdx.x * TALLY_THREADS + threadIdx.x; k < n_old; k += gridDim.x * TALLY_THREADS) {
        const TallySlot e = old_slots[k];
        if (!tally_is_published(e.state)) continue;
        uint32_t i = distinct_home(e.hash, slot_mask);
        bool placed = false;
        for (uint32_t probes = 0; probes <= slot_mask; ++probes, i = (i + 1) & slot_mask) {
            if (atomicCAS(&slots[i].state, TALLY_EMPTY, e.state) == TALLY_EMPTY) {
                slots[i].hash = e.hash; slots[i].text = e.text; slots[i].count = e.count;
                placed = true;
                break;
            }
        }
        if (!placed) atomicOr(&ctr->error, 2u);
    }
}

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_export(const TallySlot* slots, uint32_t n_slots, TallyExport* out, uint32_t out_cap, TallyCounters* ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    for (uint32_t base = wave * 64u; base < n_slots; base += n_waves * 64u) {
        const uint32_t k = base + lane;
        TallySlot e{};
        if (k < n_slots) e = slots[k];
        const bool live = k < n_slots && tally_is_published(e.state);
        const unsigned long long mask = __ballot(live);
        if (mask == 0) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&ctr->n_export, (uint32_t)__popcll(mask));
        at = __shfl(at, 0) + (uint32_t)__popcll(mask & below);
        if (live && at < out_cap) {
            TallyExport x;
            x.count = e.count; x.text = e.text; x.item_type = tally_state_type(e.state); x.slot = k;
            out[at] = x;
        }
    }
}

// one wave per text: `list[w]` names the pool bytes and where they go in `dst`
__global__ __launch_bounds__(TALLY_THREADS) void k_tally_gather(const uint8_t* pool, unsigned long long pool_cap, const TallyGather* list, uint32_t n, uint8_t* dst, unsigned long long dst_cap) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    for (uint32_t w = wave; w < n; w += n_waves) {
        const TallyGather g = list[w];
        const unsigned long long off = distinct_text_off(g.text);
        const uint32_t len = distinct_text_len(g.text);
        if (off + len > pool_cap || g.dst_off + len > dst_cap) continue;
        for (uint32_t o = lane; o < len; o += 64u) dst[g.dst_off + o] = pool[off + o];
    }
}

unsigned long long env_u64(const char* name, unsigned long long dflt) {
    const char* e = getenv(name);
    return e && *e ? strtoull(e, nullptr, 10) : dflt;
}

int grid_for_items(size_t n, size_t per_block) { return (int)std::max<size_t>(1, std::min<size_t>((n + per_block - 1) / per_block, 2048)); }

template <class T>
struct Scratch {   // a device allocation that lives as long as one call
    T* p = nullptr;
    explicit Scratch(size_t n) { if (n) MXY_HIP(hipMalloc((void**)&p, n * sizeof(T))); }
    ~Scratch() { if (p) (void)hipFree(p); }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
};

}  // namespace

HitTally::HitTally() {
    // tests only: small initial sizes (growth while entries are live), fewer hash bits (equal hashes, long probe runs)
    init_slots_ = distinct_slots_for(0, std::min<unsigned long long>(env_u64("MATCHY_AMD_TALLY_SLOTS", 1ull << 16), 1ull << 31));
    init_pool_ = std::max<unsigned long long>(distinct_pool_bytes((uint32_t)std::min<unsigned long long>(env_u64("MATCHY_AMD_TALLY_POOL_BYTES", 1ull << 20), 1ull << 30)), 64);
    hash_bits_ = (uint32_t)std::min<unsigned long long>(env_u64("MATCHY_AMD_TALLY_HASH_BITS", 64), 64);
}

HitTally::~HitTally() {
    if (slots_) (void)hipFree(slots_);
    if (pool_) (void)hipFree(pool_);
    if (ctr_) (void)hipFree(ctr_);
    if (ctr_host_) (void)hipHostFree(ctr_host_);
    if (slot_of_) (void)hipFree(slot_of_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
}

void HitTally::reset() {
    if (slots_) MXY_HIP(hipMemset(slots_, 0, n_slots_ * sizeof(TallySlot)));
    if (ctr_) MXY_HIP(hipMemset(ctr_, 0, sizeof(TallyCounters)));
    distinct_ = 0; matches_ = 0; pool_used_ = 0;
    events_ = Events{};
    poisoned_ = false;
}

void HitTally::ensure_counters() {
    if (ctr_) return;
    MXY_HIP(hipMalloc((void**)&ctr_, sizeof(TallyCounters)));
    MXY_HIP(hipMemset(ctr_, 0, sizeof(TallyCounters)));
    MXY_HIP(hipHostMalloc((void**)&ctr_host_, sizeof(TallyCounters), hipHostMallocDefault));
}

// A table that stays at most half full with `entries` keys. The new table is allocated before the old one is let go: a failed
// allocation leaves the tally as it was.
void HitTally::ensure_table(uint64_t entries, hipStream_t stream) {
    if (slots_ && 2 * entries <= n_slots_) return;
    const unsigned long long want = distinct_slots_for(entries, slots_ ? 2 * n_slots_ : init_slots_);
    if (want > (1ull << 31)) throw HipError{"hit tally: more than 2^30 distinct values"};
    TallySlot* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want * sizeof(TallySlot));
    if (e != hipSuccess) throw HipError{"hit tally: cannot allocate a table of " + std::to_string(want) + " slots: " + hipGetErrorString(e)};
    e = hipMemsetAsync(fresh, 0, want * sizeof(TallySlot), stream);
    if (e == hipSuccess && slots_ && distinct_) {
        hipLaunchKernelGGL(k_tally_rehash, dim3(grid_for_items(n_slots_, TALLY_THREADS)), dim3(TALLY_THREADS), 0, stream, (const TallySlot*)slots_, (uint32_t)n_slots_,
                           fresh, (uint32_t)(want - 1), ctr_);
        e = hipGetLastError();
        ++events_.rehashes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{std::string("hit tally: rehash: ") + hipGetErrorString(e)}; }
    if (slots_) (void)hipFree(slots_);
    slots_ = fresh; n_slots_ = want;
}

// A pool of at least `want` bytes with the old pool's content.
void HitTally::grow_pool(unsigned long long want, hipStream_t stream) {
    // whole pages, except for the tiny pools of the tests (MATCHY_AMD_TALLY_POOL_BYTES), which stay as small as asked so that they fill up
    want = want >= 4096 ? (want + 4095) & ~4095ull : distinct_pool_bytes((uint32_t)want);
    if (want > (1ull << 40)) throw HipError{"hit tally: text pool beyond 1 TiB"};
    uint8_t* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want);
    if (e != hipSuccess) throw HipError{"hit tally: cannot allocate a text pool of " + std::to_string(want) + " bytes: " + hipGetErrorString(e)};
    if (pool_) {
        e = hipMemcpyAsync(fresh, pool_, pool_cap_, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{std::string("hit tally: pool copy: ") + hipGetErrorString(e)}; }
        (void)hipFree(pool_);
    }
    pool_ = fresh; pool_cap_ = want;
}

void HitTally::add(const uint8_t* log, uint32_t len, const FinalHit* final, uint32_t n_final, const uint2* c4, uint32_t n_c4, hipStream_t stream) {
    last_ms_ = claim_ms_ = publish_ms_ = 0;
    events_ = Events{};
    if (poisoned_) throw HipError{"hit tally: inconsistent after an earlier error; call matchy_scanner_reset_tally"};
    if (!final) n_final = 0;
    if (!c4) n_c4 = 0;
    const size_t n = (size_t)n_final + n_c4;
    if (n == 0 || !log || !len) return;
    if (n > TALLY_MAX_RECORDS) throw HipError{"hit tally: more than 2^32 records in one batch"};
    ensure_counters();
    // the second counter line: counted records, new entries, pending winners, error bits (pool_used, in the first, lives as long as the tally)
    MXY_HIP(hipMemsetAsync(&ctr_->n_counted, 0, 128, stream));
    if (profile_) {
        for (auto& e : ev_) if (!e) MXY_HIP(hipEventCreate(&e));
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    // everything that can fail for lack of memory comes first: up to here and through these the tally is untouched
    ensure_table(distinct_ + n, stream);
    if (!pool_) grow_pool(init_pool_, stream);
    if (slot_of_n_ < n) {
        if (slot_of_) (void)hipFree(slot_of_);
        slot_of_ = nullptr; slot_of_n_ = 0;
        MXY_HIP(hipMalloc((void**)&slot_of_, (n + n / 4 + 1024) * sizeof(uint32_t)));
        slot_of_n_ = n + n / 4 + 1024;
    }

    poisoned_ = true;   // until the batch is in: a throw below leaves claimed slots behind
    TallyParams p{};
    p.log = log; p.len = len;
    p.recs = final; p.n_recs = n_final; p.c4 = c4; p.n_c4 = n_c4;
    p.slots = slots_; p.slot_mask = (uint32_t)(n_slots_ - 1);
    p.pool = pool_; p.pool_cap = pool_cap_;
    p.hash_mask = distinct_hash_mask(hash_bits_);
    p.slot_of = slot_of_; p.slot_of_cap = (uint32_t)std::min<size_t>(slot_of_n_, 0xFFFFFFFFu);
    p.ctr = ctr_;
    hipEvent_t claim_begin = ev_[0];
    if (profile_ && events_.rehashes) { MXY_HIP(hipEventRecord(ev_[2], stream)); claim_begin = ev_[2]; }   // the claim interval starts behind the rehash
    hipLaunchKernelGGL(k_tally_claim, dim3(grid_for_items(n, TALLY_CLAIM_ITEMS)), dim3(TALLY_THREADS), 0, stream, p);
    check_launch("k_tally_claim");
    if (profile_) {
        MXY_HIP(hipEventRecord(ev_[1], stream));
        MXY_HIP(hipEventSynchronize(ev_[1]));
        MXY_HIP(hipEventElapsedTime(&claim_ms_, claim_begin, ev_[1]));
    }
    // The publish pass, again behind every pool regrow. A pass that finds the pool full has counted its whole demand in pool_used, and
    // the winners it left pending reserve once more in the next pass: a pool of demand + (demand - start of the batch) bytes holds that
    // pass whatever it stored before, so one regrow settles a batch; MAX_REGROWS bounds the loop against a miscount.
    constexpr int MAX_REGROWS = 3;
    const int grid = grid_for_items(n, TALLY_THREADS);
    for (int attempt = 0;; ++attempt) {
        hipLaunchKernelGGL(k_tally_publish, dim3(grid), dim3(TALLY_THREADS), 0, stream, p);
        check_launch("k_tally_publish");
        if (profile_) MXY_HIP(hipEventRecord(ev_[2], stream));
        MXY_HIP(hipMemcpyAsync(ctr_host_, ctr_, sizeof(TallyCounters), hipMemcpyDeviceToHost, stream));
        MXY_HIP(hipStreamSynchronize(stream));
        if (ctr_host_->error) throw HipError{"hit tally: table full (the table was sized for fewer records than the batch holds)"};
        if (ctr_host_->n_pending == 0) break;
        if (attempt >= MAX_REGROWS) throw HipError{"hit tally: text pool still full after regrowing"};
        const unsigned long long demand = ctr_host_->pool_used;
        grow_pool(std::max(2 * pool_cap_, demand + (demand - pool_used_)), stream);
        ++events_.pool_regrows;
        p.pool = pool_; p.pool_cap = pool_cap_;
        MXY_HIP(hipMemsetAsync(&ctr_->n_pending, 0, sizeof(uint32_t), stream));
    }
    if (profile_) {
        MXY_HIP(hipEventElapsedTime(&publish_ms_, ev_[1], ev_[2]));
        MXY_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[2]));
    }
    pool_used_ = ctr_host_->pool_used;
    distinct_ += ctr_host_->n_new;
    matches_ += ctr_host_->n_counted;
    events_.direct_adds = ctr_host_->n_direct;
    events_.new_entries = ctr_host_->n_new;
    poisoned_ = false;
}

// A report path: three scratch allocations and three waits per read-out. `stream` need not be the stream of the scans: add() returns
// with its stream synchronised, so everything a read-out sees was complete before it was called (Scanner::tally_top passes the null stream).
void HitTally::top(size_t limit, std::vector<TallyEntry>& out, hipStream_t stream) {
    out.clear();
    if (poisoned_) throw HipError{"hit tally: inconsistent after an earlier error; call matchy_scanner_reset_tally"};
    if (!slots_ || !distinct_) return;
    // every published entry's count, text word and type: 24 bytes each
    const size_t cap = (size_t)distinct_;
    Scratch<TallyExport> ex_dev(cap);
    MXY_HIP(hipMemsetAsync(&ctr_->n_export, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_tally_export, dim3(grid_for_items(n_slots_, TALLY_THREADS)), dim3(TALLY_THREADS), 0, stream, (const TallySlot*)slots_, (uint32_t)n_slots_, ex_dev.p,
                       (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), ctr_);
    check_launch("k_tally_export");
    MXY_HIP(hipMemcpyAsync(ctr_host_, ctr_, sizeof(TallyCounters), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    if (ctr_host_->n_export != distinct_) throw HipError{"hit tally: the table holds " + std::to_string(ctr_host_->n_export) + " entries, " + std::to_string(distinct_) + " were published"};
    std::vector<TallyExport> ex(cap);
    MXY_HIP(hipMemcpyAsync(ex.data(), ex_dev.p, cap * sizeof(TallyExport), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    // the texts of the entries that can be among the first `limit`, in one buffer and one copy
    const std::vector<uint32_t> chosen = tally_select(ex, limit);
    std::vector<TallyGather> list(chosen.size());
    unsigned long long bytes = 0;
    for (size_t i = 0; i < chosen.size(); ++i) {
        list[i].text = ex[chosen[i]].text; list[i].dst_off = bytes;
        bytes += distinct_text_len(ex[chosen[i]].text);
    }
    std::vector<uint8_t> texts((size_t)bytes);
    if (bytes) {
        Scratch<TallyGather> list_dev(list.size());
        Scratch<uint8_t> dst_dev((size_t)bytes);
        MXY_HIP(hipMemcpyAsync(list_dev.p, list.data(), list.size() * sizeof(TallyGather), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_tally_gather, dim3(grid_for_items(list.size(), TALLY_THREADS / 64)), dim3(TALLY_THREADS), 0, stream, (const uint8_t*)pool_, pool_cap_,
                           (const TallyGather*)list_dev.p, (uint32_t)list.size(), dst_dev.p, bytes);
        check_launch("k_tally_gather");
        MXY_HIP(hipMemcpyAsync(texts.data(), dst_dev.p, (size_t)bytes, hipMemcpyDeviceToHost, stream));
        MXY_HIP(hipStreamSynchronize(stream));
    }
    out.resize(chosen.size());
    for (size_t i = 0; i < chosen.size(); ++i) {
        const TallyExport& x = ex[chosen[i]];
        out[i].text.assign(reinterpret_cast<const char*>(texts.data()) + list[i].dst_off, distinct_text_len(x.text));
        out[i].item_type = (uint8_t)x.item_type;
        out[i].count = x.count;
    }
    tally_order(out, limit);
}

}  // namespace mxy
