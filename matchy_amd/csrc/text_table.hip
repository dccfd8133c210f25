// The host side of the device text table (text_table.h) and its rehash kernel: allocation, growth with live entries, the
// publish-until-stored loop and the poisoned protocol, once for the distinct-text set and the hit tally.
#include "text_table.h"

#include <algorithm>
#include <cstdlib>
#include <string>


namespace mxy {

namespace {

constexpr uint32_t TEXT_THREADS = 256;

// published slots of the old table, all four words, into the new one (filled with the empty word); the keys are distinct, so nothing
// is compared. Between batches only.
__global__ __launch_bounds__(TEXT_THREADS) void k_text_rehash(const TextSlot* old_slots, uint32_t n_old, TextSlot* slots, uint32_t slot_mask, unsigned long long empty,
                                                             TextCounters* ctr) {
    for (uint32_t k = blockIdx.x * TEXT_THREADS + threadIdx.x; k < n_old; k += gridDim.x * TEXT_THREADS) {
        const TextSlot e = old_slots[k];
        if (!text_is_published(e.state, empty)) continue;
        uint32_t i = text_home(e.hash, slot_mask);
        bool placed = false;
        for (uint32_t probes = 0; probes <= slot_mask; ++probes, i = (i + 1) & slot_mask) {
            if (atomicCAS(&slots[i].state, empty, e.state) == empty) {
                slots[i].hash = e.hash; slots[i].text = e.text; slots[i].aux = e.aux;
                placed = true;
                break;
            }
        }
        if (!placed) atomicOr(&ctr->error, 2u);
    }
}

unsigned long long env_u64(const std::string& name, unsigned long long dflt) {
    const char* e = getenv(name.c_str());
    return e && *e ? strtoull(e, nullptr, 10) : dflt;
}

}  // namespace

TextTable::TextTable(const TextTableOwner& owner) : own_(owner) {
    // tests only: small initial sizes (growth while entries are live), fewer hash bits (equal hashes, long probe runs)
    const std::string env = own_.env_prefix;
    init_slots_ = text_slots_for(0, std::min<unsigned long long>(env_u64(env + "SLOTS", 1ull << 16), 1ull << 31));
    init_pool_ = std::max<unsigned long long>(text_pool_bytes((uint32_t)std::min<unsigned long long>(env_u64(env + "POOL_BYTES", 1ull << 20), 1ull << 30)), 64);
    hash_bits_ = (uint32_t)std::min<unsigned long long>(env_u64(env + "HASH_BITS", 64), 64);
}

void TextTable::reset() {
    if (slots_.p) MXY_HIP(hipMemset(slots_.p, (int)(own_.empty & 0xFF), slots_.n * sizeof(TextSlot)));
    if (ctr_.p) MXY_HIP(hipMemset(ctr_.p, 0, sizeof(TextCounters)));
    count_ = 0; pool_used_ = 0;
    poisoned_ = false;
}

void TextTable::check() const {
    if (poisoned_) throw HipError{std::string(own_.who) + ": inconsistent after an earlier error; call " + own_.reset_call};
}

void TextTable::start_batch(hipStream_t stream) {
    if (!ctr_host_.p) {
        ctr_.alloc(1);
        MXY_HIP(hipMemset(ctr_.p, 0, sizeof(TextCounters)));
        ctr_host_.alloc(1);
    }
    // the second counter line (pool_used, in the first, lives as long as the table)
    MXY_HIP(hipMemsetAsync(&ctr_.p->n_counted, 0, 128, stream));
}

// The new table is allocated before the old one is let go: a failed allocation leaves the table as it was.
void TextTable::ensure_table(uint64_t entries, hipStream_t stream, uint32_t& rehashes) {
    if (slots_.p && 2 * entries <= slots_.n) return;
    const std::string who = own_.who;
    const unsigned long long want = text_slots_for(entries, slots_.p ? 2 * slots_.n : init_slots_);
    if (want > (1ull << 31)) throw HipError{who + ": more than 2^30 distinct " + own_.entries};
    DevBuf<TextSlot> fresh;   // released on every way out: the new table while it is incomplete, the old one behind the swap
    hipError_t e = hipMalloc((void**)&fresh.p, want * sizeof(TextSlot));
    if (e != hipSuccess) throw HipError{who + ": cannot allocate a table of " + std::to_string(want) + " slots: " + hipGetErrorString(e)};
    fresh.n = want;
    e = hipMemsetAsync(fresh.p, (int)(own_.empty & 0xFF), want * sizeof(TextSlot), stream);
    if (e == hipSuccess && slots_.p && count_) {
        const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((slots_.n + TEXT_THREADS - 1) / TEXT_THREADS, own_.rehash_grid_cap));
        hipLaunchKernelGGL(k_text_rehash, dim3(grid), dim3(TEXT_THREADS), 0, stream, (const TextSlot*)slots_.p, (uint32_t)slots_.n, fresh.p, (uint32_t)(want - 1), own_.empty, ctr_.p);
        e = hipGetLastError();
        ++rehashes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) throw HipError{who + ": rehash: " + hipGetErrorString(e)};
    slots_.swap(fresh);
}

// A pool of at least `want` bytes with the old pool's content: whole pages, except for the tiny pools of the tests
// (MATCHY_AMD_*_POOL_BYTES), which stay as small as asked so that they fill up.
void TextTable::grow_pool(unsigned long long want, hipStream_t stream) {
    const std::string who = own_.who;
    want = want >= 4096 ? (want + 4095) & ~4095ull : text_pool_bytes((uint32_t)want);
    if (want > (1ull << 40)) throw HipError{who + ": text pool beyond 1 TiB"};
    DevBuf<uint8_t> fresh;   // as in ensure_table
    hipError_t e = hipMalloc((void**)&fresh.p, want);
    if (e != hipSuccess) throw HipError{who + ": cannot allocate a text pool of " + std::to_string(want) + " bytes: " + hipGetErrorString(e)};
    fresh.n = want;
    if (pool_.p) {
        e = hipMemcpyAsync(fresh.p, pool_.p, pool_.n, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) throw HipError{who + ": pool copy: " + hipGetErrorString(e)};
    }
    pool_.swap(fresh);
}

uint32_t TextTable::reserve(uint64_t entries, size_t n_items, hipStream_t stream) {
    uint32_t rehashes = 0;
    ensure_table(entries, stream, rehashes);
    if (!pool_.p) grow_pool(init_pool_, stream);
    if (slot_of_.n < n_items) slot_of_.alloc(n_items + n_items / 4 + 1024);
    return rehashes;
}

TextTableView TextTable::open() {
    poisoned_ = true;   // until close(): a throw in between leaves claimed slots behind
    return view();
}

TextTableView TextTable::view() const {
    TextTableView t{};
    t.slots = slots_.p; t.slot_mask = (uint32_t)(slots_.n - 1);
    t.pool = pool_.p; t.pool_cap = pool_.n;
    t.hash_mask = text_hash_mask(hash_bits_);
    t.slot_of = slot_of_.p; t.slot_of_cap = (uint32_t)std::min<size_t>(slot_of_.n, 0xFFFFFFFFu);
    t.ctr = ctr_.p;
    return t;
}

void TextTable::fetch_counters(hipStream_t stream) {
    MXY_HIP(hipMemcpyAsync(ctr_host_.p, ctr_.p, sizeof(TextCounters), hipMemcpyDeviceToHost, stream));
    MXY_HIP(hipStreamSynchronize(stream));
}

// A pass that finds the pool full has counted its whole demand in pool_used, and the winners it left pending reserve once more in the
// next pass: a pool of demand + (demand - start of the batch) bytes holds that pass whatever it stored before, so one regrow settles a
// batch; MAX_REGROWS bounds the loop against a miscount.
uint32_t TextTable::publish(const std::function<void()>& launch, TextTableView& view, hipStream_t stream) {
    constexpr uint32_t MAX_REGROWS = 3;
    for (uint32_t regrows = 0;; ++regrows) {
        launch();
        fetch_counters(stream);
        if (ctr_host_.p->error) throw HipError{std::string(own_.who) + ": table full (" + own_.full_reason + ")"};
        if (ctr_host_.p->n_pending == 0) return regrows;
        if (regrows >= MAX_REGROWS) throw HipError{std::string(own_.who) + ": text pool still full after regrowing"};
        const unsigned long long demand = ctr_host_.p->pool_used;
        grow_pool(std::max<unsigned long long>(2 * pool_.n, demand + (demand - pool_used_)), stream);
        view.pool = pool_.p; view.pool_cap = pool_.n;
        MXY_HIP(hipMemsetAsync(&ctr_.p->n_pending, 0, sizeof(uint32_t), stream));
    }
}

void TextTable::close() {
    pool_used_ = ctr_host_.p->pool_used;
    count_ += ctr_host_.p->n_new;
    poisoned_ = false;
}

}  // namespace mxy
