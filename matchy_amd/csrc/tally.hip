// Hit tally on the GPU (`matchy match --tally`, matchy_scanner_set_tally): how often every distinct matched value hit, kept in device
// memory across batches in a device text table (text_table.h: slots, probe walk, publish step, growth) whose fourth slot word is the
// count, and read out as a top-N list. It is fed from the final records of a scan while the batch is still resident, so nothing but
// counters and the rows of the report ever crosses the bus.
//
// The key is (item type, matched text): an XXH64 of the text seeded with the type picks the home slot; equality is decided by comparing
// the type and then the bytes. The 16-byte records and the compact IPv4 records of a batch form one index space. The claim word is the
// record's index + 1: all holders of a slot have identical type and bytes, so any of them will do and no order key is needed.
//
//   k_tally_claim     one lane per record walks the probe run of its key and then counts for the slot it ended in, through the
//                     workgroup's LDS aggregator (lds_aggregator.h: slot index -> count, one leader round): a workgroup covers at least
//                     1024 records, so a million hits on one address end in about a thousand global atomics (by construction, not by
//                     measurement).
//   k_tally_publish   the record whose index is still in its slot stores the text through the table's publish step, which marks the
//                     slot published with the type. The count word is not touched.
//   k_tally_export    the published slots as a dense array {count, text word, type, slot}, one atomic per wave.
//   k_tally_gather    the texts of a host-chosen list of entries into one contiguous buffer (one wave per text).
#include "tally.h"

#include <algorithm>
#include <string>

#include "lds_aggregator.h"

namespace mxy {

namespace {

constexpr uint32_t TALLY_THREADS = 256;
constexpr uint32_t TALLY_CLAIM_ITEMS = 1024;   // records per workgroup of k_tally_claim at least (while the grid allows): what one flush of the aggregator covers
// 256 entries of a key word and a count word are 2 KiB, two of the 1280-byte granules LDS is handed out in: eight workgroups of 256
// threads (all the wave slots of a CU hold) take 20 KiB of its LDS.
using TallyAgg = LdsAggregator<8, 4, 1>;

struct TallyParams {
    const uint8_t* log;
    uint32_t len;
    const FinalHit* recs;      // entries [0, n_recs) of the batch's index space
    uint32_t n_recs;
    const uint2* c4;           // entries [n_recs, n_recs + n_c4)
    uint32_t n_c4;
    TextTableView t;
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

// record `idx` of the batch as a key of the table (text_table.h)
struct TallyKey {
    static constexpr unsigned long long EMPTY = TALLY_EMPTY;
    const TallyParams& p;
    const uint8_t* text;
    uint32_t len, type, idx;
    __device__ __forceinline__ TallyKey(const TallyParams& p_, const Rec& r, uint32_t idx_) : p(p_), text(p_.log + r.start), len(r.len), type(r.type), idx(idx_) {}
    __device__ __forceinline__ unsigned long long hash(unsigned long long mask) const { return tally_hash(text, len, type, mask); }
    __device__ __forceinline__ unsigned long long claim_word() const { return tally_claim_word(idx); }
    __device__ __forceinline__ unsigned long long published_word() const { return tally_published(type); }
    __device__ __forceinline__ bool same_key(unsigned long long o) const { return tally_state_type(o) == type; }
    __device__ __forceinline__ bool holder_is_me(unsigned long long o) const {
        const uint32_t hidx = tally_claim_index(o);
        if (hidx >= p.n_recs + p.n_c4) return false;
        const Rec holder = d_rec(p, hidx);
        return holder.type == type && holder.len == len && tally_usable(holder.start, holder.len, p.len) && d_bytes_equal(p.log + holder.start, text, len);
    }
    __device__ __forceinline__ void join(unsigned long long*, unsigned long long) const {}
};

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_claim(const TallyParams p) {
    __shared__ uint32_t agg_keys[TallyAgg::SLOTS];
    __shared__ uint32_t agg_counts[TallyAgg::SLOTS];
    TallyAgg::clear(agg_keys, agg_counts, TALLY_THREADS);
    __syncthreads();
    const uint32_t n = p.n_recs + p.n_c4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the counting below is wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        uint32_t found = TEXT_NO_SLOT;
        if (idx < n) {
            const Rec r = d_rec(p, idx);
            if (tally_usable(r.start, r.len, p.len)) {
                const TallyKey k(p, r, idx);
                if (d_text_probe(p.t, k, k.hash(p.t.hash_mask), found) == Probe::Full) atomicOr(&p.t.ctr->error, 1u);
            }
            if (idx < p.t.slot_of_cap) p.t.slot_of[idx] = found;
        }
        // count: one add per lane that found a slot; an add the aggregator had no room for goes straight to the global word
        const unsigned long long counting = __ballot(found != TEXT_NO_SLOT);
        if (counting == 0) continue;
        const uint32_t direct = TallyAgg::count(agg_keys, agg_counts, counting, found, lane);
        if (direct) atomicAdd(&p.t.slots[found].aux, (unsigned long long)direct);
        const unsigned long long past = __ballot(direct != 0);
        if (lane == (uint32_t)__ffsll((long long)counting) - 1u) {
            atomicAdd(&p.t.ctr->n_counted, (unsigned long long)__popcll(counting));
            if (past) atomicAdd(&p.t.ctr->n_direct, (uint32_t)__popcll(past));
        }
    }
    __syncthreads();
    TallyAgg::flush(agg_keys, agg_counts, TALLY_THREADS, [&](uint32_t k, uint32_t c) {
        if (k <= p.t.slot_mask) atomicAdd(&p.t.slots[k].aux, (unsigned long long)c);
    });
}

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_publish(const TallyParams p) {
    const uint32_t n = p.n_recs + p.n_c4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    // every lane of a wave takes every turn of this loop: the publish step is wave-wide
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const uint32_t idx = base + lane;
        Rec r{0, 0, 0};
        uint32_t slot = TEXT_NO_SLOT;
        bool win = false;
        if (idx < n && idx < p.t.slot_of_cap) {
            slot = p.t.slot_of[idx];
            if (slot <= p.t.slot_mask) {
                r = d_rec(p, idx);
                win = d_slot_state(&p.t.slots[slot].state) == tally_claim_word(idx) && tally_usable(r.start, r.len, p.len);
            }
        }
        uint32_t rank;
        d_text_publish(p.t, win, slot, TallyKey(p, r, idx), lane, rank);
    }
}

__global__ __launch_bounds__(TALLY_THREADS) void k_tally_export(const TextSlot* slots, uint32_t n_slots, TallyExport* out, uint32_t out_cap, TextCounters* ctr) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t wave = (blockIdx.x * TALLY_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * TALLY_THREADS) >> 6;
    for (uint32_t base = wave * 64u; base < n_slots; base += n_waves * 64u) {
        const uint32_t k = base + lane;
        TextSlot e{};
        if (k < n_slots) e = slots[k];
        const bool live = k < n_slots && tally_is_published(e.state);
        const unsigned long long mask = __ballot(live);
        if (mask == 0) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&ctr->n_export, (uint32_t)__popcll(mask));
        at = __shfl(at, 0) + (uint32_t)__popcll(mask & below);
        if (live && at < out_cap) {
            TallyExport x;
            x.count = e.aux; x.text = e.text; x.item_type = tally_state_type(e.state); x.slot = k;
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
        const unsigned long long off = text_word_off(g.text);
        const uint32_t len = text_word_len(g.text);
        if (off + len > pool_cap || g.dst_off + len > dst_cap) continue;
        for (uint32_t o = lane; o < len; o += 64u) dst[g.dst_off + o] = pool[off + o];
    }
}

int grid_for_items(size_t n, size_t per_block) { return (int)std::max<size_t>(1, std::min<size_t>((n + per_block - 1) / per_block, 2048)); }

}  // namespace

// tests only: MATCHY_AMD_TALLY_SLOTS, MATCHY_AMD_TALLY_POOL_BYTES, MATCHY_AMD_TALLY_HASH_BITS
constexpr TextTableOwner TALLY_OWNER = {"hit tally", "values", "matchy_scanner_reset_tally", "the table was sized for fewer records than the batch holds",
                                        "MATCHY_AMD_TALLY_", TALLY_EMPTY, 2048};

HitTally::HitTally() : table_(TALLY_OWNER) {}

void HitTally::reset() {
    table_.reset();
    matches_ = 0;
    events_ = Events{};
}

void HitTally::add(const uint8_t* log, uint32_t len, const FinalHit* final, uint32_t n_final, const uint2* c4, uint32_t n_c4, hipStream_t stream) {
    last_ms_ = claim_ms_ = publish_ms_ = 0;
    events_ = Events{};
    table_.check();
    if (!final) n_final = 0;
    if (!c4) n_c4 = 0;
    const size_t n = (size_t)n_final + n_c4;
    if (n == 0 || !log || !len) return;
    if (n > TALLY_MAX_RECORDS) throw HipError{"hit tally: more than 2^32 records in one batch"};
    table_.start_batch(stream);
    if (profile_) {
        for (Event& e : ev_) e.create();
        MXY_HIP(hipEventRecord(ev_[0], stream));
    }
    // everything that can fail for lack of memory comes first: up to here and through these the tally is untouched
    events_.rehashes = table_.reserve(table_.count() + n, n, stream);

    TallyParams p{};
    p.log = log; p.len = len;
    p.recs = final; p.n_recs = n_final; p.c4 = c4; p.n_c4 = n_c4;
    p.t = table_.open();
    hipEvent_t claim_begin = ev_[0];
    if (profile_ && events_.rehashes) { MXY_HIP(hipEventRecord(ev_[2], stream)); claim_begin = ev_[2]; }   // the claim interval starts behind the rehash
    hipLaunchKernelGGL(k_tally_claim, dim3(grid_for_items(n, TALLY_CLAIM_ITEMS)), dim3(TALLY_THREADS), 0, stream, p);
    check_launch("k_tally_claim");
    if (profile_) {
        MXY_HIP(hipEventRecord(ev_[1], stream));
        MXY_HIP(hipEventSynchronize(ev_[1]));
        MXY_HIP(hipEventElapsedTime(&claim_ms_, claim_begin, ev_[1]));
    }
    const int grid = grid_for_items(n, TALLY_THREADS);
    events_.pool_regrows = table_.publish([&] {
        hipLaunchKernelGGL(k_tally_publish, dim3(grid), dim3(TALLY_THREADS), 0, stream, p);
        check_launch("k_tally_publish");
        if (profile_) MXY_HIP(hipEventRecord(ev_[2], stream));
    }, p.t, stream);
    if (profile_) {
        MXY_HIP(hipEventElapsedTime(&publish_ms_, ev_[1], ev_[2]));
        MXY_HIP(hipEventElapsedTime(&last_ms_, ev_[0], ev_[2]));
    }
    const TextCounters& c = table_.host_counters();
    matches_ += c.n_counted;
    events_.direct_adds = c.n_direct;
    events_.new_entries = c.n_new;
    table_.close();
}

// A report path: three scratch allocations and three waits per read-out. `stream` need not be the stream of the scans: add() returns
// with its stream synchronised, so everything a read-out sees was complete before it was called (Scanner::tally_top passes the null stream).
void HitTally::top(size_t limit, std::vector<TallyEntry>& out, hipStream_t stream) {
    out.clear();
    table_.check();
    const uint64_t distinct = table_.count();
    if (!distinct) return;
    const TextTableView t = table_.view();
    // every published entry's count, text word and type: 24 bytes each
    const size_t cap = (size_t)distinct;
    DevBuf<TallyExport> ex_dev;   // the device allocations of a read-out live as long as the call
    ex_dev.alloc(cap);
    MXY_HIP(hipMemsetAsync(&t.ctr->n_export, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_tally_export, dim3(grid_for_items((size_t)t.slot_mask + 1, TALLY_THREADS)), dim3(TALLY_THREADS), 0, stream, (const TextSlot*)t.slots, t.slot_mask + 1, ex_dev.p,
                       (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu), t.ctr);
    check_launch("k_tally_export");
    table_.fetch_counters(stream);
    const uint32_t n_export = table_.host_counters().n_export;
    if (n_export != distinct) throw HipError{"hit tally: the table holds " + std::to_string(n_export) + " entries, " + std::to_string(distinct) + " were published"};
    std::vector<TallyExport> ex(cap);
    MXY_HIP(hipMemcpyAsync(ex.data(), ex_dev.p, cap * sizeof(TallyExport), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
    // the texts of the entries that can be among the first `limit`, in one buffer and one copy
    const std::vector<uint32_t> chosen = tally_select(ex, limit);
    std::vector<TallyGather> list(chosen.size());
    unsigned long long bytes = 0;
    for (size_t i = 0; i < chosen.size(); ++i) {
        list[i].text = ex[chosen[i]].text; list[i].dst_off = bytes;
        bytes += text_word_len(ex[chosen[i]].text);
    }
    std::vector<uint8_t> texts((size_t)bytes);
    if (bytes) {
        DevBuf<TallyGather> list_dev;
        DevBuf<uint8_t> dst_dev;
        list_dev.alloc(list.size()); dst_dev.alloc((size_t)bytes);
        MXY_HIP(hipMemcpyAsync(list_dev.p, list.data(), list.size() * sizeof(TallyGather), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_tally_gather, dim3(grid_for_items(list.size(), TALLY_THREADS / 64)), dim3(TALLY_THREADS), 0, stream, (const uint8_t*)t.pool, t.pool_cap,
                           (const TallyGather*)list_dev.p, (uint32_t)list.size(), dst_dev.p, bytes);
        check_launch("k_tally_gather");
        MXY_HIP(hipMemcpyAsync(texts.data(), dst_dev.p, (size_t)bytes, hipMemcpyDeviceToHost, stream));
        MXY_HIP(hipStreamSynchronize(stream));
    }
    out.resize(chosen.size());
    for (size_t i = 0; i < chosen.size(); ++i) {
        const TallyExport& x = ex[chosen[i]];
        out[i].text.assign(reinterpret_cast<const char*>(texts.data()) + list[i].dst_off, text_word_len(x.text));
        out[i].item_type = (uint8_t)x.item_type;
        out[i].count = x.count;
    }
    tally_order(out, limit);
}

}  // namespace mxy
