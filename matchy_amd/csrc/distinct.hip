// Distinct candidate texts on the GPU (`matchy extract --unique`, matchy_amd_extractor_set_unique): an exact set of byte strings that
// lives in device memory across batches — an open-addressing table of 32-byte slots (linear probing, at most half full) and a pool that
// holds the text of every entry, so that a later batch, whose log is another buffer, can compare against it.
//
// A 64-bit XXH64 of the text picks the home slot; equality is always decided by comparing bytes. The state of a slot is its `order`
// word (distinct.h), the only word several lanes write in one launch:
//
//   k_distinct_claim    one lane per candidate of the batch. It walks the probe run of its text: a published slot (an earlier batch)
//                       with the same hash, length and bytes makes it a duplicate; a slot claimed in this batch holds the order key of
//                       a candidate of this batch, whose bytes are in the same log — equal bytes: the lane joins the slot with a 64-bit
//                       atomicMin of its own key (skipped when the key it read is smaller already: a million copies of one address
//                       cost a million loads and a handful of atomics); an empty slot is claimed with a compare-and-swap of the key.
//                       Different texts never share a slot, whatever their hashes, so there is no retry round.
//   k_distinct_publish  the candidate whose key is still in its slot is the first of its text in the batch, by (start, type rank). The
//                       winners of a wave reserve pool space with one atomic, copy their text, fill in the slot, mark it published and
//                       append their record to the output list (one atomic per wave). A winner that finds the pool full stays claimed
//                       and is counted; the host grows the pool and runs the pass again for exactly those.
//   k_distinct_rehash   moves the published slots into a larger table. Runs between batches only, when the candidates of the next batch
//                       could fill the table beyond one half.
#include "distinct.h"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "engine.h"

namespace mxy {

namespace {

constexpr uint32_t DISTINCT_THREADS = 256;

struct DistinctParams {
    const uint8_t* log;
    uint32_t len;
    const Candidate* list_a;   // entries [0, n_a) of the batch's index space
    uint32_t n_a;
    const Candidate* list_b;   // entries [n_a, n_a + n_b)
    uint32_t n_b;
    DistinctSlot* slots;
    uint32_t slot_mask;
    uint8_t* pool;
    unsigned long long pool_cap;
    unsigned long long hash_mask;
    uint32_t* slot_of;
    Candidate* out;
    uint32_t out_cap;
    DistinctCounters* ctr;
};

__device__ __forceinline__ Candidate d_cand(const DistinctParams& p, uint32_t i) { return i < p.n_a ? p.list_a[i] : p.list_b[i - p.n_a]; }
// a real candidate whose text lies inside the batch
__device__ __forceinline__ bool d_usable(const DistinctParams& p, const Candidate& c) {
    if (c.len_type == 0xFFFFFFFFu) return false;
    const uint32_t n = c.len_type & 0xFFFFFFu;
    return c.start < p.len && n <= p.len - c.start;
}
__device__ __forceinline__ unsigned long long d_order(const unsigned long long* w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

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

__global__ __launch_bounds__(DISTINCT_THREADS) void k_distinct_claim(const DistinctParams p) {
    const uint32_t n = p.n_a + p.n_b;
    for (uint32_t idx = blockIdx.x * DISTINCT_THREADS + threadIdx.x; idx < n; idx += gridDim.x * DISTINCT_THREADS) {
        const Candidate c = d_cand(p, idx);
        uint32_t found = DISTINCT_NO_SLOT;
        if (d_usable(p, c)) {
            const uint32_t len = c.len_type & 0xFFFFFFu;
            const uint8_t* text = p.log + c.start;
            const unsigned long long h = xxh64(text, len, 0) & p.hash_mask;
            const unsigned long long key = distinct_order_key(c.start, c.len_type >> 24, idx);
            uint32_t i = distinct_home(h, p.slot_mask);
            bool placed = false;
            for (uint32_t probes = 0; probes <= p.slot_mask; ++probes, i = (i + 1) & p.slot_mask) {
                DistinctSlot* s = &p.slots[i];
                unsigned long long o = d_order(&s->order);
                if (o == DISTINCT_EMPTY) {
                    o = atomicCAS(&s->order, DISTINCT_EMPTY, key);
                    if (o == DISTINCT_EMPTY) { found = i; placed = true; break; }
                }
                if (!distinct_is_key(o)) {   // published by an earlier batch: its words and its pool bytes are final
                    if (s->hash != h) continue;
                    const unsigned long long tw = s->text;
                    if (distinct_text_len(tw) == len && d_bytes_equal(p.pool + distinct_text_off(tw), text, len)) { placed = true; break; }   // seen before
                    continue;
                }
                // claimed in this batch by a candidate of this batch: the same text joins it, any other walks on
                const Candidate holder = d_cand(p, distinct_key_index(o));
                if ((holder.len_type & 0xFFFFFFu) == len && d_bytes_equal(p.log + holder.start, text, len)) {
                    if (key < o) atomicMin(&s->order, key);   // `order` only falls: a key above what was read cannot win
                    found = i; placed = true;
                    break;
                }
            }
            if (!placed) atomicOr(&p.ctr->error, 1u);   // a full table: the host keeps it half empty, so this is a miscount
        }
        p.slot_of[idx] = found;
    }
}

__global__ __launch_bounds__(DISTINCT_THREADS) void k_distinct_publish(const DistinctParams p) {
    const uint32_t n = p.n_a + p.n_b;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t wave = (blockIdx.x * DISTINCT_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * DISTINCT_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the reservations below are wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        Candidate c{};
        uint32_t slot = DISTINCT_NO_SLOT, len = 0;
        bool win = false;
        if (idx < n) {
            slot = p.slot_of[idx];
            if (slot != DISTINCT_NO_SLOT) {
                c = d_cand(p, idx);
                len = c.len_type & 0xFFFFFFu;
                win = d_order(&p.slots[slot].order) == distinct_order_key(c.start, c.len_type >> 24, idx);
            }
        }
        const unsigned long long winners = __ballot(win);
        if (winners == 0) continue;
        // pool space: inclusive prefix of the winners' (padded) lengths over the wave, one atomic for the sum
        const uint32_t bytes = win ? (uint32_t)distinct_pool_bytes(len) : 0u;
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
            const uint8_t* text = p.log + c.start;
            uint8_t* dst = p.pool + off;   // 8-byte aligned; the padding bytes behind the text are never read
            uint32_t o = 0;
            for (; o + 8 <= len; o += 8) {
                unsigned long long v;
                __builtin_memcpy(&v, text + o, 8);
                *reinterpret_cast<unsigned long long*>(dst + o) = v;
            }
            for (; o < len; ++o) dst[o] = text[o];
            DistinctSlot* s = &p.slots[slot];
            s->hash = xxh64(text, len, 0) & p.hash_mask;
            s->text = distinct_text_word(off, len);
            s->reserved = 0;
            // nobody reads hash / text / pool bytes before the next launch; the lanes of this launch only compare `order` with their own key
            __hip_atomic_store(&s->order, DISTINCT_PUBLISHED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const unsigned long long done = __ballot(stored);
        uint32_t out_base = 0;
        if (lane == 0) {
            if (done) out_base = atomicAdd(&p.ctr->n_out, (uint32_t)__popcll(done));
            if (winners & ~done) atomicAdd(&p.ctr->n_pending, (uint32_t)__popcll(winners & ~done));
        }
        out_base = __shfl(out_base, 0);
        if (stored) {
            const uint32_t o = out_base + (uint32_t)__popcll(done & below);
            if (o < p.out_cap) p.out[o] = c;
        }
    }
}

// published slots of the old table into the new one (filled with DISTINCT_EMPTY); the texts are distinct, so nothing is compared
__global__ __launch_bounds__(DISTINCT_THREADS) void k_distinct_rehash(const DistinctSlot* old_slots, uint32_t n_old, DistinctSlot* slots, uint32_t slot_mask,
                                                                      DistinctCounters* ctr) {
    for (uint32_t k = blockIdx.x * DISTINCT_THREADS + threadIdx.x; k < n_old; k += gridDim.x * DISTINCT_THREADS) {
        const DistinctSlot e = old_slots[k];
        if (e.order != DISTINCT_PUBLISHED) continue;
        uint32_t i = distinct_home(e.hash, slot_mask);
        bool placed = false;
        for (uint32_t probes = 0; probes <= slot_mask; ++probes, i = (i + 1) & slot_mask) {
            if (atomicCAS(&slots[i].order, DISTINCT_EMPTY, DISTINCT_PUBLISHED) == DISTINCT_EMPTY) {
                slots[i].hash = e.hash; slots[i].text = e.text; slots[i].reserved = 0;
                placed = true;
                break;
            }
        }
        if (!placed) atomicOr(&ctr->error, 2u);
    }
}

unsigned long long env_u64(const char* name, unsigned long long dflt) {
    const char* e = getenv(name);
    return e && *e ? strtoull(e, nullptr, 10) : dflt;
}

int grid_for_items(size_t n) { return (int)std::min<size_t>((n + DISTINCT_THREADS - 1) / DISTINCT_THREADS, 4096); }

}  // namespace

DistinctSet::DistinctSet() {
    // tests only: small initial sizes (growth while entries are live), fewer hash bits (equal hashes, long probe runs)
    init_slots_ = distinct_slots_for(0, std::min<unsigned long long>(env_u64("MATCHY_AMD_DISTINCT_SLOTS", 1ull << 16), 1ull << 31));
    init_pool_ = std::max<unsigned long long>(distinct_pool_bytes((uint32_t)std::min<unsigned long long>(env_u64("MATCHY_AMD_DISTINCT_POOL_BYTES", 1ull << 20), 1ull << 30)), 64);
    hash_bits_ = (uint32_t)std::min<unsigned long long>(env_u64("MATCHY_AMD_DISTINCT_HASH_BITS", 64), 64);
}

DistinctSet::~DistinctSet() {
    if (slots_) (void)hipFree(slots_);
    if (pool_) (void)hipFree(pool_);
    if (ctr_) (void)hipFree(ctr_);
    if (ctr_host_) (void)hipHostFree(ctr_host_);
    if (slot_of_) (void)hipFree(slot_of_);
    if (out_dev_) (void)hipFree(out_dev_);
    for (auto& e : ev_) if (e) (void)hipEventDestroy(e);
}

void DistinctSet::reset() {
    if (slots_) MXY_HIP(hipMemset(slots_, 0xFF, n_slots_ * sizeof(DistinctSlot)));
    if (ctr_) MXY_HIP(hipMemset(ctr_, 0, sizeof(DistinctCounters)));
    count_ = 0; pool_used_ = 0;
    poisoned_ = false;
}

// A table that stays at most half full with `entries` texts. The new table is allocated before the old one is let go: a failed
// allocation leaves the set as it was.
void DistinctSet::ensure_table(uint64_t entries, hipStream_t stream) {
    if (slots_ && 2 * entries <= n_slots_) return;
    const unsigned long long want = distinct_slots_for(entries, slots_ ? 2 * n_slots_ : init_slots_);
    if (want > (1ull << 31)) throw HipError{"distinct set: more than 2^30 distinct texts"};
    DistinctSlot* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want * sizeof(DistinctSlot));
    if (e != hipSuccess) throw HipError{"distinct set: cannot allocate a table of " + std::to_string(want) + " slots: " + hipGetErrorString(e)};
    e = hipMemsetAsync(fresh, 0xFF, want * sizeof(DistinctSlot), stream);
    if (e == hipSuccess && slots_ && count_) {
        hipLaunchKernelGGL(k_distinct_rehash, dim3(grid_for_items(n_slots_)), dim3(DISTINCT_THREADS), 0, stream, (const DistinctSlot*)slots_, (uint32_t)n_slots_,
                           fresh, (uint32_t)(want - 1), ctr_);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{std::string("distinct set: rehash: ") + hipGetErrorString(e)}; }
    if (slots_) (void)hipFree(slots_);
    slots_ = fresh; n_slots_ = want;
}

// A pool of at least `want` bytes with the old pool's content.
void DistinctSet::grow_pool(unsigned long long want, hipStream_t stream) {
    want = (want + 4095) & ~4095ull;
    if (want > (1ull << 40)) throw HipError{"distinct set: text pool beyond 1 TiB"};
    uint8_t* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want);
    if (e != hipSuccess) throw HipError{"distinct set: cannot allocate a text pool of " + std::to_string(want) + " bytes: " + hipGetErrorString(e)};
    if (pool_) {
        e = hipMemcpyAsync(fresh, pool_, pool_cap_, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{std::string("distinct set: pool copy: ") + hipGetErrorString(e)}; }
        (void)hipFree(pool_);
    }
    pool_ = fresh; pool_cap_ = want;
}

void DistinctSet::filter(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                         std::vector<Candidate>& out, hipStream_t stream) {
    out.clear();
    last_ms_ = 0;
    if (poisoned_) throw HipError{"distinct set: inconsistent after an earlier error; call matchy_amd_extractor_reset_unique"};
    const size_t n = (size_t)n_a + n_b;
    if (n == 0 || cand_true == 0) return;
    if (len > DISTINCT_MAX_LEN) throw HipError{"distinct set: batch longer than 1 GiB"};
    if (n >= DISTINCT_MAX_INDEX) throw HipError{"distinct set: more than 2^29 candidate list entries in one batch"};
    if (!ctr_) {
        MXY_HIP(hipMalloc((void**)&ctr_, sizeof(DistinctCounters)));
        MXY_HIP(hipMemset(ctr_, 0, sizeof(DistinctCounters)));
        MXY_HIP(hipHostMalloc((void**)&ctr_host_, sizeof(DistinctCounters), hipHostMallocDefault));
    }
    // the second counter line: survivors, pending winners, error bits (pool_used, in the first, lives as long as the set)
    MXY_HIP(hipMemsetAsync(&ctr_->n_out, 0, 128, stream));
    // everything that can fail for lack of memory comes first: up to here and through these the set is untouched
    ensure_table(count_ + cand_true, stream);
    if (!pool_) grow_pool(init_pool_, stream);
    if (slot_of_n_ < n) {
        if (slot_of_) (void)hipFree(slot_of_);
        slot_of_ = nullptr; slot_of_n_ = 0;
        MXY_HIP(hipMalloc((void**)&slot_of_, (n + n / 4 + 1024) * sizeof(uint32_t)));
        slot_of_n_ = n + n / 4 + 1024;
    }
    if (out_n_ < cand_true) {
        if (out_dev_) (void)hipFree(out_dev_);
        out_dev_ = nullptr; out_n_ = 0;
        MXY_HIP(hipMalloc((void**)&out_dev_, ((size_t)cand_true + cand_true / 4 + 1024) * sizeof(Candidate)));
        out_n_ = (size_t)cand_true + cand_true / 4 + 1024;
    }
    if (profile_) for (auto& e : ev_) if (!e) MXY_HIP(hipEventCreate(&e));

    poisoned_ = true;   // until the batch is in: a throw below leaves claimed slots behind
    DistinctParams p{};
    p.log = log; p.len = len;
    p.list_a = list_a; p.n_a = n_a; p.list_b = list_b; p.n_b = n_b;
    p.slots = slots_; p.slot_mask = (uint32_t)(n_slots_ - 1);
    p.pool = pool_; p.pool_cap = pool_cap_;
    p.hash_mask = distinct_hash_mask(hash_bits_);
    p.slot_of = slot_of_;
    p.out = out_dev_; p.out_cap = (uint32_t)std::min<size_t>(out_n_, 0xFFFFFFFFu);
    p.ctr = ctr_;
    const int grid = grid_for_items(n);
    if (profile_) MXY_HIP(hipEventRecord(ev_[0], stream));
    hipLaunchKernelGGL(k_distinct_claim, dim3(grid), dim3(DISTINCT_THREADS), 0, stream, p);
    check_launch("k_distinct_claim");
    // The publish pass, again behind every pool regrow. A pass that finds the pool full has counted its whole demand in pool_used, and
    // the winners it left pending reserve once more in the next pass: a pool of demand + (demand - start of the batch) bytes holds that
    // pass whatever it stored before, so one regrow settles a batch; MAX_REGROWS bounds the loop against a miscount.
    constexpr int MAX_REGROWS = 3;
    for (int attempt = 0;; ++attempt) {
        hipLaunchKernelGGL(k_distinct_publish, dim3(grid), dim3(DISTINCT_THREADS), 0, stream, p);
        check_launch("k_distinct_publish");
        if (profile_) MXY_HIP(hipEventRecord(ev_[1], stream));
        MXY_HIP(hipMemcpyAsync(ctr_host_, ctr_, sizeof(DistinctCounters), hipMemcpyDeviceToHost, stream));
        MXY_HIP(hipStreamSynchronize(stream));
        if (ctr_host_->error) throw HipError{"distinct set: table full (candidate count of the batch was wrong)"};
        if (ctr_host_->n_pending == 0) break;
        if (attempt >= MAX_REGROWS) throw HipError{"distinct set: text pool still full after regrowing"};
        const unsigned long long demand = ctr_host_->pool_used;
        grow_pool(std::max(2 * pool_cap_, demand + (demand - pool_used_)), stream);
        p.pool = pool_; p.pool_cap = pool_cap_;
        MXY_HIP(hipMemsetAsync(&ctr_->n_pending, 0, sizeof(uint32_t), stream));
    }
    const uint32_t n_out = ctr_host_->n_out;
    if (n_out > p.out_cap) throw HipError{"distinct set: more survivors than candidates"};
    out.resize(n_out);
    if (n_out) MXY_HIP(hipMemcpyAsync(out.data(), out_dev_, (size_t)n_out * sizeof(Candidate), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    if (profile_) MXY_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
    pool_used_ = ctr_host_->pool_used;
    count_ += n_out;
    poisoned_ = false;
}

}  // namespace mxy
