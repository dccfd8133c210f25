// The host side of the device text table (text_table.h) and its rehash kernel: allocation, growth with live entries, the
// publish-until-stored loop and the poisoned protocol, once for the distinct-text set and the hit tally.
#include "text_table.h"

#include <algorithm>
#include <cstdlib>
#include <string>

#include "engine.h"

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

TextTable::~TextTable() {
    if (slots_) (void)hipFree(slots_);
    if (pool_) (void)hipFree(pool_);
    if (ctr_) (void)hipFree(ctr_);
    if (ctr_host_) (void)hipHostFree(ctr_host_);
    if (slot_of_) (void)hipFree(slot_of_);
}

void TextTable::reset() {
    if (slots_) MXY_HIP(hipMemset(slots_, (int)(own_.empty & 0xFF), n_slots_ * sizeof(TextSlot)));
    if (ctr_) MXY_HIP(hipMemset(ctr_, 0, sizeof(TextCounters)));
    count_ = 0; pool_used_ = 0;
    poisoned_ = false;
}

void TextTable::check() const {
    if (poisoned_) throw HipError{std::string(own_.who) + ": inconsistent after an earlier error; call " + own_.reset_call};
}

void TextTable::start_batch(hipStream_t stream) {
    if (!ctr_) {
        MXY_HIP(hipMalloc((void**)&ctr_, sizeof(TextCounters)));
        MXY_HIP(hipMemset(ctr_, 0, sizeof(TextCounters)));
        MXY_HIP(hipHostMalloc((void**)&ctr_host_, sizeof(TextCounters), hipHostMallocDefault));
    }
    // the second counter line (pool_used, in the first, lives as long as the table)
    MXY_HIP(hipMemsetAsync(&ctr_->n_counted, 0, 128, stream));
}

// The new table is allocated before the old one is let go: a failed allocation leaves the table as it was.
void TextTable::ensure_table(uint64_t entries, hipStream_t stream, uint32_t& rehashes) {
    if (slots_ && 2 * entries <= n_slots_) return;
    const std::string who = own_.who;
    const unsigned long long want = text_slots_for(entries, slots_ ? 2 * n_slots_ : init_slots_);
    if (want > (1ull << 31)) throw HipError{who + ": more than 2^30 distinct " + own_.entries};
    TextSlot* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want * sizeof(TextSlot));
    if (e != hipSuccess) throw HipError{who + ": cannot allocate a table of " + std::to_string(want) + " slots: " + hipGetErrorString(e)};
    e = hipMemsetAsync(fresh, (int)(own_.empty & 0xFF), want * sizeof(TextSlot), stream);
    if (e == hipSuccess && slots_ && count_) {
        const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((n_slots_ + TEXT_THREADS - 1) / TEXT_THREADS, own_.rehash_grid_cap));
        hipLaunchKernelGGL(k_text_rehash, dim3(grid), dim3(TEXT_THREADS), 0, stream, (const TextSlot*)slots_, (uint32_t)n_slots_, fresh, (uint32_t)(want - 1), own_.empty, ctr_);
        e = hipGetLastError();
        ++rehashes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{who + ": rehash: " + hipGetErrorString(e)}; }
    if (slots_) (void)hipFree(slots_);
    slots_ = fresh; n_slots_ = want;
}

// A pool of at least `want` bytes with the old pool's content: whole pages, except for the tiny pools of the tests
// (MATCHY_AMD_*_POOL_BYTES), which stay as small as asked so that they fill up.
void TextTable::grow_pool(unsigned long long want, hipStream_t stream) {
    const std::string who = own_.who;
    want = want >= 4096 ? (want + 4095) & ~4095ull : text_pool_bytes((uint32_t)want);
    if (want > (1ull << 40)) throw HipError{who + ": text pool beyond 1 TiB"};
    uint8_t* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, want);
    if (e != hipSuccess) throw HipError{who + ": cannot allocate a text pool of " + std::to_string(want) + " bytes: " + hipGetErrorString(e)};
    if (pool_) {
        e = hipMemcpyAsync(fresh, pool_, pool_cap_, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(fresh); throw HipError{who + ": pool copy: " + hipGetErrorString(e)}; }
        (void)hipFree(pool_);
    }
    pool_ = fresh; pool_cap_ = want;
}

uint32_t TextTable::reserve(uint64_t entries, size_t n_items, hipStream_t stream) {
    uint32_t rehashes = 0;
    ensure_table(entries, stream, rehashes);
    if (!pool_) grow_pool(init_pool_, stream);
    if (slot_of_n_ < n_items) {
        if (slot_of_) (void)hipFree(slot_of_);
        slot_of_ = nullptr; slot_of_n_ = 0;
        MXY_HIP(hipMalloc((void**)&slot_of_, (n_items + n_items / 4 + 1024) * sizeof(uint32_t)));
        slot_of_n_ = n_items + n_items / 4 + 1024;
    }
    return rehashes;
}

TextTableView TextTable::open() {
    poisoned_ = true;   // until close(): a throw in between leaves claimed slots behind
    return view();
}

TextTableView TextTable::view() const {
    TextTableView t{};
    t.slots = slots_; t.slot_mask = (uint32_t)(n_slots_ - 1);
    t.pool = pool_; t.pool_cap = pool_cap_;
    t.hash_mask = text_hash_mask(hash_bits_);
    t.slot_of = slot_of_; t.slot_of_cap = (uint32_t)std::min<size_t>(slot_of_n_, 0xFFFFFFFFu);
    t.ctr = ctr_;
    return t;
}

void TextTable::fetch_counters(hipStream_t stream) {
    MXY_HIP(hipMemcpyAsync(ctr_host_, ctr_, sizeof(TextCounters), hipMemcpyDeviceToHost, stream));
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
        if (ctr_host_->error) throw HipError{std::string(own_.who) + ": table full (" + own_.full_reason + ")"};
        if (ctr_host_->n_pending == 0) return regrows;
        if (regrows >= MAX_REGROWS) throw HipError{std::string(own_.who) + ": text pool still full after regrowing"};
        const unsigned long long demand = ctr_host_->pool_used;
        grow_pool(std::max(2 * pool_cap_, demand + (demand - pool_used_)), stream);
        view.pool = pool_; view.pool_cap = pool_cap_;
        MXY_HIP(hipMemsetAsync(&ctr_->n_pending, 0, sizeof(uint32_t), stream));
    }
}

void TextTable::close() {
    pool_used_ = ctr_host_->pool_used;
    count_ += ctr_host_->n_new;
    poisoned_ = false;
}

}  // namespace mxy
