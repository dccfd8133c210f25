// Distinct candidate texts on the GPU (`matchy extract --unique`, matchy_amd_extractor_set_unique): an exact set of byte strings that
// lives in device memory across batches, in a device text table (text_table.h: slots, probe walk, publish step, growth).
//
// The key is the text alone: a 64-bit XXH64 of it (seed 0) picks the home slot; equality is always decided by comparing bytes. The
// claim word is an order key (distinct.h), so that of the candidates of one text in a batch the least by (start, type rank) stays:
//
//   k_distinct_claim    one lane per candidate of the batch walks the probe run of its text. A published slot with its bytes makes it a
//                       duplicate; a slot claimed in this batch by a candidate with the same bytes is joined with a 64-bit atomicMin
//                       of the lane's own key (skipped when the key it read is smaller already: a million copies of one address cost
//                       a million loads and a handful of atomics); an empty slot is claimed with the key.
//   k_distinct_publish  the candidate whose key is still in its slot is the first of its text in the batch. The winners are published
//                       by the table's publish step and append their record to the output list at the rank that step hands back: a
//                       survivor is exactly a newly published entry.
#include "distinct.h"

#include <algorithm>
#include <string>


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
    TextTableView t;
    Candidate* out;
    uint32_t out_cap;
};

__device__ __forceinline__ Candidate d_cand(const DistinctParams& p, uint32_t i) { return i < p.n_a ? p.list_a[i] : p.list_b[i - p.n_a]; }
// a real candidate whose text lies inside the batch
__device__ __forceinline__ bool d_usable(const DistinctParams& p, const Candidate& c) {
    if (c.len_type == 0xFFFFFFFFu) return false;
    const uint32_t n = c.len_type & 0xFFFFFFu;
    return c.start < p.len && n <= p.len - c.start;
}

// candidate `idx` of the batch as a key of the table (text_table.h)
struct DistinctKey {
    static constexpr unsigned long long EMPTY = DISTINCT_EMPTY;
    const DistinctParams& p;
    const uint8_t* text;
    uint32_t len, start, type, idx;
    __device__ __forceinline__ DistinctKey(const DistinctParams& p_, const Candidate& c, uint32_t idx_)
        : p(p_), text(p_.log + c.start), len(c.len_type & 0xFFFFFFu), start(c.start), type(c.len_type >> 24), idx(idx_) {}
    __device__ __forceinline__ unsigned long long hash(unsigned long long mask) const { return xxh64(text, len, 0) & mask; }
    __device__ __forceinline__ unsigned long long claim_word() const { return distinct_order_key(start, type, idx); }
    __device__ __forceinline__ unsigned long long published_word() const { return DISTINCT_PUBLISHED; }
    __device__ __forceinline__ bool same_key(unsigned long long) const { return true; }
    __device__ __forceinline__ bool holder_is_me(unsigned long long o) const {
        const Candidate holder = d_cand(p, distinct_key_index(o));
        return (holder.len_type & 0xFFFFFFu) == len && d_bytes_equal(p.log + holder.start, text, len);
    }
    // `state` only falls: a key above what was read cannot win
    __device__ __forceinline__ void join(unsigned long long* state, unsigned long long o) const { if (claim_word() < o) atomicMin(state, claim_word()); }
};

__global__ __launch_bounds__(DISTINCT_THREADS) void k_distinct_claim(const DistinctParams p) {
    const uint32_t n = p.n_a + p.n_b;
    for (uint32_t idx = blockIdx.x * DISTINCT_THREADS + threadIdx.x; idx < n; idx += gridDim.x * DISTINCT_THREADS) {
        const Candidate c = d_cand(p, idx);
        uint32_t found = TEXT_NO_SLOT;
        if (d_usable(p, c)) {
            const DistinctKey k(p, c, idx);
            const Probe end = d_text_probe(p.t, k, k.hash(p.t.hash_mask), found);
            if (end == Probe::Published) found = TEXT_NO_SLOT;   // seen before
            if (end == Probe::Full) atomicOr(&p.t.ctr->error, 1u);
        }
        p.t.slot_of[idx] = found;
    }
}

__global__ __launch_bounds__(DISTINCT_THREADS) void k_distinct_publish(const DistinctParams p) {
    const uint32_t n = p.n_a + p.n_b;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * DISTINCT_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * DISTINCT_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the publish step is wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        Candidate c{};
        uint32_t slot = TEXT_NO_SLOT;
        if (idx < n) {
            slot = p.t.slot_of[idx];
            if (slot != TEXT_NO_SLOT) c = d_cand(p, idx);
        }
        const DistinctKey k(p, c, idx);
        const bool win = slot != TEXT_NO_SLOT && d_slot_state(&p.t.slots[slot].state) == k.claim_word();
        uint32_t rank;
        if (d_text_publish(p.t, win, slot, k, lane, rank) && rank < p.out_cap) p.out[rank] = c;
    }
}

int grid_for_items(size_t n) { return (int)std::min<size_t>((n + DISTINCT_THREADS - 1) / DISTINCT_THREADS, 4096); }

}  // namespace

// tests only: MATCHY_AMD_DISTINCT_SLOTS, MATCHY_AMD_DISTINCT_POOL_BYTES, MATCHY_AMD_DISTINCT_HASH_BITS
constexpr TextTableOwner DISTINCT_OWNER = {"distinct set", "texts", "matchy_amd_extractor_reset_unique", "candidate count of the batch was wrong",
                                           "MATCHY_AMD_DISTINCT_", DISTINCT_EMPTY, 4096};

DistinctSet::DistinctSet() : table_(DISTINCT_OWNER) {}

void DistinctSet::reset() { table_.reset(); }

// claim + publish of one batch: the survivors in out_dev_, their number returned. `false` in `open`: the batch had nothing to filter and
// the table was not opened; otherwise the caller closes the table once it has what it wants from out_dev_.
uint32_t DistinctSet::run(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                          hipStream_t stream, bool& open) {
    open = false;
    last_ms_ = 0;
    table_.check();
    const size_t n = (size_t)n_a + n_b;
    if (n == 0 || cand_true == 0) return 0;
    if (len > DISTINCT_MAX_LEN) throw HipError{"distinct set: batch longer than 1 GiB"};
    if (n >= DISTINCT_MAX_INDEX) throw HipError{"distinct set: more than 2^29 candidate list entries in one batch"};
    table_.start_batch(stream);
    // everything that can fail for lack of memory comes first: up to here and through these the set is untouched
    table_.reserve(table_.count() + cand_true, n, stream);
    if (out_dev_.n < cand_true) out_dev_.alloc((size_t)cand_true + cand_true / 4 + 1024);
    if (profile_) for (Event& e : ev_) e.create();

    DistinctParams p{};
    p.log = log; p.len = len;
    p.list_a = list_a; p.n_a = n_a; p.list_b = list_b; p.n_b = n_b;
    p.t = table_.open();
    p.out = out_dev_.p; p.out_cap = (uint32_t)std::min<size_t>(out_dev_.n, 0xFFFFFFFFu);
    const int grid = grid_for_items(n);
    if (profile_) MXY_HIP(hipEventRecord(ev_[0], stream));
    hipLaunchKernelGGL(k_distinct_claim, dim3(grid), dim3(DISTINCT_THREADS), 0, stream, p);
    check_launch("k_distinct_claim");
    table_.publish([&] {
        hipLaunchKernelGGL(k_distinct_publish, dim3(grid), dim3(DISTINCT_THREADS), 0, stream, p);
        check_launch("k_distinct_publish");
        if (profile_) MXY_HIP(hipEventRecord(ev_[1], stream));
    }, p.t, stream);
    const uint32_t n_out = table_.host_counters().n_new;
    if (n_out > p.out_cap) throw HipError{"distinct set: more survivors than candidates"};
    open = true;
    return n_out;
}

void DistinctSet::filter(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                         std::vector<Candidate>& out, hipStream_t stream) {
    out.clear();
    bool open;
    const uint32_t n_out = run(log, len, list_a, n_a, list_b, n_b, cand_true, stream, open);
    if (!open) return;
    out.resize(n_out);
    if (n_out) MXY_HIP(hipMemcpyAsync(out.data(), out_dev_.p, (size_t)n_out * sizeof(Candidate), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    if (profile_) MXY_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));
    table_.close();
}

uint32_t DistinctSet::filter_device(const uint8_t* log, uint32_t len, const Candidate* list_a, uint32_t n_a, const Candidate* list_b, uint32_t n_b, uint32_t cand_true,
                                    hipStream_t stream) {
    bool open;
    const uint32_t n_out = run(log, len, list_a, n_a, list_b, n_b, cand_true, stream, open);
    if (!open) return 0;
    if (profile_) MXY_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[1]));   // the publish step has waited for the stream
    table_.close();
    return n_out;
}

}  // namespace mxy
