// GPU: the wave-level work-list writers of device_common.h against a sequential host model (driver: tests/test_gpu_list_writers.py).
//
// Every writer the kernels instantiate is driven by a tiny kernel of its own: W waves make R converged append calls each, the emitting
// lanes of a call given by a 64-bit mask per (wave, round) that the host drew from a seeded generator; a stored value encodes
// (wave, round, lane), so every entry is unique and traceable. Each driver ends with the writer's end-of-work call.
//
// The reference is the model below, written from the comments of the writers (it includes none of their code): per wave the list of
// reservations in the order the wave makes them, each with its size and the entries it receives, in the order they are written; slots
// behind the entries hold the sentinel. Where a reservation lands is decided by the atomics of all waves, so the comparison is free of
// order between reservations and exact within one: the reservations must TILE [0, counter) — the slot behind one reservation starts
// another one, found by its first entry.
//
// The output is allocated as max(capacity, demand) + GUARD slots and filled with a poison value that is neither an entry nor a
// sentinel: a writer that misses a capacity test stores inside the allocation, where the host finds it, and never faults.
//
// Checked for every case (writer x wave count x capacity):
//   1. counter == the model's total of reserved slots (the exact demand a regrow is sized from; for the writers whose reservation
//      size depends on their flush history this pins that history)
//   2. every slot >= capacity still holds poison
//   3. every slot < min(counter, capacity) holds an entry or the sentinel, never poison
//   4. the reservations tile [0, min(counter, capacity)): each holds the model's entries in the model's order, then sentinels; with
//      capacity >= counter that is every emitted entry exactly once
//   5. DomWriter: the slot it returns is 0xFFFFFFFF exactly for lanes that do not emit and for slots >= capacity; only plane 0 is
//      written; a wave that owns a static chunk and never emits leaves it all sentinels (k_anchor's end-of-work sequence)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "device_common.h"

using namespace mxy;

// stage sizes of k_anchor.hip's CandWriter / RareWriter (the Python driver checks that they still are what k_anchor.hip says)
constexpr uint32_t CAND_STAGE = 16, RARE_STAGE = 8;
constexpr uint32_t GUARD = 4096;        // slots behind the larger of capacity and demand
constexpr uint32_t POISON = 0xDEADBEEFu;
constexpr uint32_t WPB = 4;             // waves per workgroup (256 threads)
constexpr uint32_t NONE = 0xFFFFFFFFu;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FATAL %s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(3); } } while (0)

// ------------------------------------------------------------------------------------------------ values
// id > 0 in the first dword of every type; no field of an entry looks like the sentinel or the poison (ids stay below 2^24)
__host__ __device__ inline uint32_t entry_id(uint32_t wave, uint32_t R, uint32_t round, uint32_t lane) { return (wave * R + round) * 64u + lane + 1u; }

template <class T> struct Val;
template <> struct Val<uint32_t> {
    __host__ __device__ static uint32_t make(uint32_t id) { return id; }
    static bool is_sentinel(const uint32_t& v) { return v == 0xFFFFFFFFu; }
    static uint32_t sentinel() { return 0xFFFFFFFFu; }
};
template <> struct Val<uint2> {
    __host__ __device__ static uint2 make(uint32_t id) { return make_uint2(id, (id << 8) | 1u); }
    static bool is_sentinel(const uint2& v) { return (v.y & 0xFFu) == 0xFFu; }   // kind 0xFF
    static uint2 sentinel() { return make_uint2(0xFFFFFFFFu, 0xFFu); }
};
template <> struct Val<RareAnchor> {
    __host__ __device__ static RareAnchor make(uint32_t id) { return RareAnchor{id, (id << 8) | 2u}; }
    static bool is_sentinel(const RareAnchor& v) { return (v.len_kind & 0xFFu) == 0xFFu; }
    static RareAnchor sentinel() { return RareAnchor{0xFFFFFFFFu, 0xFFu}; }
};
template <> struct Val<Candidate> {
    __host__ __device__ static Candidate make(uint32_t id) { return Candidate{id, id ^ 0x05000000u, ~id, 2u}; }
    static bool is_sentinel(const Candidate& v) { return v.len_type == 0xFFFFFFFFu; }
    static Candidate sentinel() { return Candidate{0u, 0xFFFFFFFFu, 0u, 0u}; }
};
template <> struct Val<Hit> {
    __host__ __device__ static Hit make(uint32_t id) {
        Hit h{};
        h.cand = id; h.a = ~id; h.ids_off = id * 3u; h.n_globs = (uint16_t)id; h.kind = 3; h.prefix_len = (uint8_t)(id >> 5);
        h.start = id + 7u; h.len_type = id ^ 0x0A000000u;
        return h;
    }
    static bool is_sentinel(const Hit& v) { return v.kind == 0xFF; }
    static Hit sentinel() { Hit h{}; h.kind = 0xFF; return h; }
};
static_assert(sizeof(Hit) == 24 && sizeof(Candidate) == 16 && sizeof(RareAnchor) == 8, "the value makers fill every byte");

template <class T> bool is_poison(const T& v) {
    uint32_t w[sizeof(T) / 4];
    memcpy(w, &v, sizeof(T));
    for (uint32_t x : w) if (x != POISON) return false;
    return true;
}
template <class T> uint32_t first_dword(const T& v) { uint32_t x; memcpy(&x, &v, 4); return x; }
template <class T> bool same(const T& a, const T& b) { return memcmp(&a, &b, sizeof(T)) == 0; }

// ------------------------------------------------------------------------------------------------ device drivers
#define WAVE_PROLOGUE \
    const uint32_t wv = threadIdx.x >> 6, wave = blockIdx.x * WPB + wv, lane = lane_id(); \
    if (wave >= W) return;
#define ROUND_EMIT(r) (((masks[(size_t)wave * R + (r)]) >> lane) & 1ull) != 0

template <class T, uint32_t CHUNK>
__global__ __launch_bounds__(256) void k_chunk(const uint64_t* masks, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter, T sentinel) {
    WAVE_PROLOGUE
    ChunkWriter<T, CHUNK> w;
    for (uint32_t r = 0; r < R; ++r) {
        const bool emit = ROUND_EMIT(r);
        w.append(emit, Val<T>::make(entry_id(wave, R, r, lane)), out, cap, counter, sentinel);
    }
    w.pad_rest(out, cap, sentinel);
}

template <class T, uint32_t CAP>
__global__ __launch_bounds__(256) void k_buffered(const uint64_t* masks, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter) {
    __shared__ T stage[WPB][CAP];
    WAVE_PROLOGUE
    BufferedWriter<T, CAP> w(stage[wv]);
    for (uint32_t r = 0; r < R; ++r) {
        const bool emit = ROUND_EMIT(r);
        w.append(emit, Val<T>::make(entry_id(wave, R, r, lane)), out, cap, counter);
    }
    w.flush(out, cap, counter);
}

template <class T, uint32_t CAP>
__global__ __launch_bounds__(256) void k_staged(const uint64_t* masks, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter, T sentinel, uint32_t chunk) {
    __shared__ T stage[WPB][CAP];
    WAVE_PROLOGUE
    StagedChunkWriter<T, CAP> w(stage[wv], chunk);
    for (uint32_t r = 0; r < R; ++r) {
        const bool emit = ROUND_EMIT(r);
        w.append(emit, Val<T>::make(entry_id(wave, R, r, lane)), out, cap, counter, sentinel);
    }
    w.finish(out, cap, counter, sentinel);
}

// the caller's part as in k_anchor: plane 0 of the returned slot gets the value; the end of the wave's work hands a static chunk the wave
// never touched to pad_rest
__global__ __launch_bounds__(256) void k_dom(const uint64_t* masks, uint32_t W, uint32_t R, uint32_t* out, uint32_t cap, uint32_t* counter, uint32_t dom_static,
                                             uint32_t dom_chunk, uint32_t* ret) {
    WAVE_PROLOGUE
    DomWriter w;
    for (uint32_t r = 0; r < R; ++r) {
        const bool emit = ROUND_EMIT(r);
        const uint32_t slot = w.reserve(emit, out, cap, [=] { return counter; }, [=] { return dom_static ? wave * dom_static : 0xFFFFFFFFu; },
                                        [=] { return dom_chunk; });
        ret[((size_t)wave * R + r) * 64 + lane] = slot;
        if (slot != 0xFFFFFFFFu) out[dom_plane_index(slot, 0)] = entry_id(wave, R, r, lane);
        __builtin_amdgcn_wave_barrier();
    }
    if (w.next == 0xFFFFFFFFu && dom_static) {
        w.next = wave * dom_static;
        w.left = dom_static;
    }
    w.pad_rest(out, cap);
}

// ------------------------------------------------------------------------------------------------ masks
struct Masks {
    uint32_t W, R;
    std::vector<uint64_t> m;
    uint64_t at(uint32_t w, uint32_t r) const { return m[(size_t)w * R + r]; }
};

static uint64_t pick_lanes(std::mt19937_64& rng, uint32_t k) {
    if (k >= 64) return ~0ull;
    uint32_t lanes[64];
    for (uint32_t i = 0; i < 64; ++i) lanes[i] = i;
    uint64_t m = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t j = i + (uint32_t)(rng() % (64 - i));
        std::swap(lanes[i], lanes[j]);
        m |= 1ull << lanes[i];
    }
    return m;
}

// What the waves do (w = wave index):
//   w == 1 (when there is more than one wave): never emits
//   w % 4 == 0, 2: a random mix of all-zero rounds, single lanes, full rounds, the stage boundaries (stage/2, stage/2 + 1, stage - 1, stage,
//       stage + 1 lanes) and random lane counts
//   other waves: `pre` full rounds (to move a history-dependent writer into the regime of the chunk), then a chunk of `chunks` filled to
//       chunk - 1 entries (full rounds and one partial round), then a round of 0, 1 or 2 lanes: the chunk ends at chunk - 1, at exactly chunk,
//       or the round does not fit (chunk + 1); all-zero rounds behind it
//   one wave alone (W == 1) does the three fills of the first chunk size one after the other, then the random mix
// The fills count entries from the first slot of a chunk, which is exact for the writers that put an append straight into the chunk:
// ChunkWriter, StagedChunkWriter (full rounds bypass its stage) and DomWriter end a chunk at chunk - 1, chunk and chunk + 1. The
// stage of a BufferedWriter holds every departure back by one round, so there the fills only steer a wave into the 256- and 2048-slot
// regimes and fill such chunks with whole stages; which boundaries its chunks end on is left to the random waves (the model follows the
// device either way, and the Python driver requires that capacities cut through chunks of both sizes).
struct MaskPlan {
    uint32_t stage;                          // stage size of the writer (0: none)
    std::vector<uint32_t> chunks, pre;       // chunk sizes to fill, full rounds in front of each
};

static void add_fill(std::vector<uint64_t>& rounds, std::mt19937_64& rng, uint32_t pre, uint32_t chunk, uint32_t extra) {
    for (uint32_t i = 0; i < pre; ++i) rounds.push_back(~0ull);
    const uint32_t body = chunk - 1;
    for (uint32_t i = 0; i < body / 64; ++i) rounds.push_back(~0ull);
    if (body % 64) rounds.push_back(pick_lanes(rng, body % 64));
    if (extra) rounds.push_back(pick_lanes(rng, extra));
}
static void add_random(std::vector<uint64_t>& rounds, std::mt19937_64& rng, uint32_t stage, uint32_t upto) {
    const uint32_t h = stage ? stage / 2 : 32u, s = stage ? stage : 32u;
    const uint32_t special[] = {h, h + 1, s > 1 ? s - 1 : 1u, s, s + 1 <= 64 ? s + 1 : 64u};
    while (rounds.size() < upto) {
        const uint32_t dice = (uint32_t)(rng() % 100);
        if (dice < 15) rounds.push_back(0);
        else if (dice < 35) rounds.push_back(1ull << (rng() % 64));
        else if (dice < 50) rounds.push_back(~0ull);
        else if (dice < 75) rounds.push_back(pick_lanes(rng, special[rng() % 5]));
        else rounds.push_back(pick_lanes(rng, 1 + (uint32_t)(rng() % 63)));
    }
}
static Masks make_masks(uint32_t W, uint32_t R, const MaskPlan& plan, uint64_t seed) {
    Masks mk{W, R, std::vector<uint64_t>((size_t)W * R, 0)};
    std::mt19937_64 rng(seed);
    for (uint32_t w = 0; w < W; ++w) {
        std::vector<uint64_t> rounds;
        if (W == 1) {
            for (uint32_t extra = 0; extra < 3; ++extra) add_fill(rounds, rng, extra == 0 ? plan.pre[0] : 0, plan.chunks[0], extra);
            add_random(rounds, rng, plan.stage, R);
        } else if (w == 1) {
            // never emits
        } else if (w % 4 == 0 || w % 4 == 2) {
            add_random(rounds, rng, plan.stage, R);
        } else {
            const size_t c = (w / 12) % plan.chunks.size();
            add_fill(rounds, rng, plan.pre[c], plan.chunks[c], (w / 4) % 3);
        }
        if (rounds.size() > R) { printf("FATAL mask plan needs %zu rounds, have %u\n", rounds.size(), R); exit(3); }
        for (size_t r = 0; r < rounds.size(); ++r) mk.m[(size_t)w * R + r] = rounds[r];
    }
    return mk;
}

// ------------------------------------------------------------------------------------------------ the host model
struct Res {
    uint32_t size = 0;
    std::vector<uint32_t> ids;   // entries in slot order from the reservation's first slot; sentinels behind them
    int64_t fixed = -1;          // first slot when the reservation is not made with an atomic (DomWriter's static chunk)
};
typedef std::vector<Res> Model;

static void lanes_of(uint64_t m, uint32_t wave, uint32_t R, uint32_t round, std::vector<uint32_t>& to) {
    for (uint32_t l = 0; l < 64; ++l) if ((m >> l) & 1) to.push_back(entry_id(wave, R, round, l));
}

// ChunkWriter: a wave reserves CHUNK slots with one atomic and fills them with the compacted entries of its appends; an append that does not
// fit into the rest of the chunk takes a new chunk; slots the wave never fills hold the sentinel.
static Model model_chunk(const Masks& mk, uint32_t CHUNK) {
    Model out;
    for (uint32_t w = 0; w < mk.W; ++w) {
        Res* cur = nullptr;
        for (uint32_t r = 0; r < mk.R; ++r) {
            const uint64_t m = mk.at(w, r);
            const uint32_t n = (uint32_t)__builtin_popcountll(m);
            if (!n) continue;
            if (!cur || cur->ids.size() + n > CHUNK) { out.emplace_back(); cur = &out.back(); cur->size = CHUNK; }
            lanes_of(m, w, mk.R, r, cur->ids);
        }
    }
    return out;
}

// BufferedWriter: entries collect in a CAP-entry stage and leave together when the next append does not fit, and at flush(). Whatever leaves
// (a drained stage; with CAP < 64 an append of more than CAP entries, directly and past the stage) takes slots from the wave's current chunk,
// or, if it does not fit there, from a new reservation: of exactly what leaves for the wave's first four departures, of 256 slots for the
// next twelve, of 2048 later (never less than what leaves). The rest of the last chunk holds the sentinel.
static Model model_buffered(const Masks& mk, uint32_t CAP) {
    Model out;
    for (uint32_t w = 0; w < mk.W; ++w) {
        Res* cur = nullptr;
        uint32_t departures = 0;
        std::vector<uint32_t> stage;
        auto leave = [&](const std::vector<uint32_t>& ids) {
            const uint32_t n = (uint32_t)ids.size();
            if (!cur || cur->ids.size() + n > cur->size) {
                const uint32_t chunk = departures < 4 ? n : (departures < 16 ? 256u : 2048u);
                out.emplace_back(); cur = &out.back(); cur->size = std::max(chunk, n);
            }
            ++departures;
            cur->ids.insert(cur->ids.end(), ids.begin(), ids.end());
        };
        for (uint32_t r = 0; r < mk.R; ++r) {
            const uint64_t m = mk.at(w, r);
            const uint32_t n = (uint32_t)__builtin_popcountll(m);
            if (!n) continue;
            std::vector<uint32_t> ids;
            lanes_of(m, w, mk.R, r, ids);
            if (CAP < 64 && n > CAP) { leave(ids); continue; }
            if (stage.size() + n > CAP) { if (!stage.empty()) leave(stage); stage.clear(); }
            stage.insert(stage.end(), ids.begin(), ids.end());
        }
        if (!stage.empty()) leave(stage);
    }
    return out;
}

// StagedChunkWriter: chunks of max(64, chunk) slots, one atomic each. Appends of at most CAP / 2 entries collect in the CAP-entry stage,
// which leaves into the current chunk (a new one if it does not fit) when the next small append does not fit into the stage; a larger
// append first sends the stage, then goes into the chunk itself: the list is in append order per wave. Unused slots hold the sentinel.
static Model model_staged(const Masks& mk, uint32_t CAP, uint32_t chunk) {
    chunk = std::max(64u, chunk);
    Model out;
    for (uint32_t w = 0; w < mk.W; ++w) {
        Res* cur = nullptr;
        std::vector<uint32_t> stage;
        auto leave = [&](const std::vector<uint32_t>& ids) {
            if (ids.empty()) return;
            if (!cur || cur->ids.size() + ids.size() > chunk) { out.emplace_back(); cur = &out.back(); cur->size = chunk; }
            cur->ids.insert(cur->ids.end(), ids.begin(), ids.end());
        };
        for (uint32_t r = 0; r < mk.R; ++r) {
            const uint64_t m = mk.at(w, r);
            const uint32_t n = (uint32_t)__builtin_popcountll(m);
            if (!n) continue;
            std::vector<uint32_t> ids;
            lanes_of(m, w, mk.R, r, ids);
            if (n > CAP / 2) { leave(stage); stage.clear(); leave(ids); continue; }
            if (stage.size() + n > CAP) { leave(stage); stage.clear(); }
            stage.insert(stage.end(), ids.begin(), ids.end());
        }
        leave(stage);
    }
    return out;
}

// DomWriter: like ChunkWriter on plane 0 of the domain list, the chunk size given by the caller (chunk_fn). With a static first chunk
// wave w owns slots [w * ANCHOR_CHUNK, (w + 1) * ANCHOR_CHUNK) without an atomic (the counter was preset to waves * ANCHOR_CHUNK), its
// later chunks are reserved. A wave that never emits still pads its static chunk (k_anchor's end of work).
static Model model_dom(const Masks& mk, uint32_t dom_static, uint32_t dom_chunk) {
    Model out;
    for (uint32_t w = 0; w < mk.W; ++w) {
        Res* cur = nullptr;
        if (dom_static) { out.emplace_back(); out.back().size = dom_static; out.back().fixed = (int64_t)w * dom_static; }
        bool first = true;
        for (uint32_t r = 0; r < mk.R; ++r) {
            const uint64_t m = mk.at(w, r);
            const uint32_t n = (uint32_t)__builtin_popcountll(m);
            if (!n) continue;
            if (first && dom_static) cur = &out.back();
            first = false;
            if (!cur || cur->ids.size() + n > cur->size) { out.emplace_back(); cur = &out.back(); cur->size = dom_chunk; }
            lanes_of(m, w, mk.R, r, cur->ids);
        }
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ comparison
struct Cell { enum Kind { POISONED, SENTINEL, ENTRY, GARBAGE } kind; uint32_t id; };

static int g_cases = 0, g_failed = 0;

struct Check {
    std::string err;
    uint32_t straddle = 0;             // size of the reservation the capacity cut through (0: none)
    std::vector<uint32_t> slot_of_id;  // filled by the walk: slot of every entry that lies below the capacity (NONE otherwise)
    std::vector<std::pair<uint32_t, uint32_t>> layout;   // (first slot, size) of the reservations found
    void fail(const char* fmt, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
        if (!err.empty()) return;
        char buf[256];
        snprintf(buf, sizeof buf, fmt, a, b, c);
        err = buf;
    }
};

// cell(slot): what slot `slot` of the list holds. `alloc` slots were allocated; `counter` is what the device counted.
static void verify(const Model& model, uint32_t max_id, uint32_t cap, uint32_t alloc, uint32_t counter, const std::function<Cell(uint32_t)>& cell, Check& ck) {
    uint64_t total = 0;
    for (const Res& r : model) total += r.size;
    if (counter != total) ck.fail("counter %llu, the model reserves %llu", counter, total);                       // 1
    for (uint32_t s = cap; s < alloc; ++s)
        if (cell(s).kind != Cell::POISONED) { ck.fail("slot %llu >= capacity %llu was written", s, cap); break; }   // 2
    const uint32_t lim = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(counter, total), cap);
    for (uint32_t s = 0; s < lim; ++s)
        if (cell(s).kind == Cell::POISONED) { ck.fail("slot %llu below min(counter, capacity) = %llu was left as it was", s, lim); break; }   // 3
    // 4: the reservations tile [0, lim)
    std::vector<int32_t> by_first(max_id + 1, -1), by_fixed;
    std::vector<char> seen(model.size(), 0);
    for (size_t i = 0; i < model.size(); ++i) {
        if (model[i].fixed >= 0) by_fixed.push_back((int32_t)i);
        else if (model[i].ids.empty()) { ck.fail("model: a reservation without entries"); return; }
        else by_first[model[i].ids[0]] = (int32_t)i;
    }
    ck.slot_of_id.assign(max_id + 1, NONE);
    uint32_t s = 0;
    while (s < lim) {
        int32_t ri = -1;
        for (int32_t f : by_fixed) if (model[f].fixed == (int64_t)s) ri = f;
        const Cell c0 = cell(s);
        if (ri < 0) {
            if (c0.kind != Cell::ENTRY || c0.id > max_id || by_first[c0.id] < 0) { ck.fail("slot %llu (kind %llu, id %llu) does not start a reservation", s, c0.kind, c0.id); return; }
            ri = by_first[c0.id];
        }
        if (seen[ri]) { ck.fail("the reservation at slot %llu appears twice", s); return; }
        seen[ri] = 1;
        const Res& r = model[ri];
        ck.layout.emplace_back(s, r.size);
        if ((uint64_t)s + r.size > cap && s < cap) ck.straddle = r.size;
        for (uint32_t k = 0; k < r.size && s + k < cap; ++k) {
            const Cell c = cell(s + k);
            if (k < r.ids.size()) {
                if (c.kind != Cell::ENTRY || c.id != r.ids[k]) { ck.fail("slot %llu: entry %llu expected, kind %llu found", s + k, r.ids[k], c.kind); return; }
                ck.slot_of_id[r.ids[k]] = s + k;
            } else if (c.kind != Cell::SENTINEL) { ck.fail("slot %llu: sentinel expected behind the %llu entries of its reservation, kind %llu found", s + k, r.ids.size(), c.kind); return; }
        }
        s += r.size;
    }
    if (cap >= total) {
        if (s != total) ck.fail("the reservations end at slot %llu, not at the counter %llu", s, total);
        for (size_t i = 0; i < model.size(); ++i) if (!seen[i]) { ck.fail("reservation %llu of the model is not in the list", i); break; }
    }
}

static void report(const std::string& name, uint32_t W, uint32_t cap, uint32_t counter, const Check& ck) {
    ++g_cases;
    if (!ck.err.empty()) ++g_failed;
    printf("CASE %s W=%u cap=%u counter=%u cut=%u %s%s\n", name.c_str(), W, cap, counter, ck.straddle, ck.err.empty() ? "OK" : "FAIL: ", ck.err.c_str());
    fflush(stdout);
}

// capacities for one (writer, masks): none over, exactly the demand, one less, 0, and one inside a reservation of every size class of the run
// (taken from where the first pass put one: with one wave that is exact, with many the next launch lands elsewhere and `cut` in the
// report says what the capacity went through)
static std::vector<uint32_t> capacities(const Model& model, const Check& first, uint32_t total) {
    std::vector<uint32_t> caps{total};
    if (total) caps.push_back(total - 1);
    caps.push_back(0);
    std::set<uint32_t> sizes;
    for (const Res& r : model) sizes.insert(r.size < 64 ? 1u : (r.size < 256 ? 64u : r.size));   // classes: < 64, < 256, each larger size
    for (uint32_t cls : sizes) {
        // a reservation of the class near the middle of the list
        uint32_t best = NONE, best_d = NONE, best_size = 0;
        for (auto& [at, size] : first.layout) {
            const uint32_t c = size < 64 ? 1u : (size < 256 ? 64u : size);
            if (c != cls || size < 2) continue;
            const uint32_t d = at > total / 2 ? at - total / 2 : total / 2 - at;
            if (d < best_d) { best_d = d; best = at; best_size = size; }
        }
        if (best != NONE) caps.push_back(best + best_size / 2);
    }
    return caps;
}

struct DeviceCase {
    uint64_t* masks = nullptr;
    uint32_t* counter = nullptr;
    void upload(const Masks& mk) {
        HIP_OK(hipMalloc(&masks, mk.m.size() * 8));
        HIP_OK(hipMemcpy(masks, mk.m.data(), mk.m.size() * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMalloc(&counter, 4));
    }
    void release() { HIP_OK(hipFree(masks)); HIP_OK(hipFree(counter)); }
};

static const uint32_t WAVES[] = {1, 4, 320};

// launch(masks, W, R, out, cap, counter)
template <class T>
static void run_flat(const std::string& name, uint64_t seed, const MaskPlan& plan, uint32_t R, const std::function<Model(const Masks&)>& model_of,
                     const std::function<void(const uint64_t*, uint32_t, uint32_t, T*, uint32_t, uint32_t*)>& launch) {
    for (uint32_t W : WAVES) {
        const Masks mk = make_masks(W, R, plan, seed++);
        const Model model = model_of(mk);
        uint64_t total64 = 0;
        for (const Res& r : model) total64 += r.size;
        const uint32_t total = (uint32_t)total64, max_id = W * R * 64u;
        DeviceCase dc;
        dc.upload(mk);
        std::vector<uint32_t> caps{total + 1000};
        for (size_t ci = 0; ci < caps.size(); ++ci) {
            const uint32_t cap = caps[ci], alloc = std::max(cap, total) + GUARD;
            T* d_out = nullptr;
            HIP_OK(hipMalloc(&d_out, (size_t)alloc * sizeof(T)));
            HIP_OK(hipMemsetD32((hipDeviceptr_t)d_out, (int)POISON, (size_t)alloc * sizeof(T) / 4));
            HIP_OK(hipMemset(dc.counter, 0, 4));
            launch(dc.masks, W, R, d_out, cap, dc.counter);
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());
            std::vector<T> h((size_t)alloc);
            uint32_t counter = 0;
            HIP_OK(hipMemcpy(h.data(), d_out, (size_t)alloc * sizeof(T), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(&counter, dc.counter, 4, hipMemcpyDeviceToHost));
            HIP_OK(hipFree(d_out));
            Check ck;
            verify(model, max_id, cap, alloc, counter, [&](uint32_t s) -> Cell {
                const T& v = h[s];
                if (is_poison(v)) return Cell{Cell::POISONED, 0};
                if (Val<T>::is_sentinel(v)) return Cell{same(v, Val<T>::sentinel()) ? Cell::SENTINEL : Cell::GARBAGE, 0};
                const uint32_t id = first_dword(v);
                return Cell{same(v, Val<T>::make(id)) ? Cell::ENTRY : Cell::GARBAGE, id};
            }, ck);
            report(name, W, cap, counter, ck);
            if (ci == 0) for (uint32_t c : capacities(model, ck, total)) caps.push_back(c);
        }
        dc.release();
    }
}

static void run_dom(const std::string& name, uint32_t dom_static, uint32_t dom_chunk) {
    const uint32_t R = 64;
    const MaskPlan plan{0, {dom_chunk, ANCHOR_CHUNK}, {0, 0}};
    uint64_t seed = 0xD0D0000u + dom_static + dom_chunk;
    for (uint32_t W : WAVES) {
        const Masks mk = make_masks(W, R, plan, seed++);
        const Model model = model_dom(mk, dom_static, dom_chunk);
        uint64_t total64 = 0;
        for (const Res& r : model) total64 += r.size;
        const uint32_t total = (uint32_t)total64, max_id = W * R * 64u;
        DeviceCase dc;
        dc.upload(mk);
        uint32_t* d_ret = nullptr;
        HIP_OK(hipMalloc(&d_ret, (size_t)max_id * 4));
        std::vector<uint32_t> caps{total + 1000};
        for (size_t ci = 0; ci < caps.size(); ++ci) {
            const uint32_t cap = caps[ci];
            const uint32_t alloc = (std::max(cap, total) + GUARD + DOM_TILE - 1) / DOM_TILE * DOM_TILE;   // whole tiles of DOM_PLANES planes
            const size_t dwords = (size_t)alloc * DOM_PLANES;
            uint32_t* d_out = nullptr;
            HIP_OK(hipMalloc(&d_out, dwords * 4));
            HIP_OK(hipMemsetD32((hipDeviceptr_t)d_out, (int)POISON, dwords));
            HIP_OK(hipMemsetD32((hipDeviceptr_t)d_ret, (int)POISON, max_id));
            const uint32_t preset = dom_static ? W * dom_static : 0u;
            HIP_OK(hipMemcpy(dc.counter, &preset, 4, hipMemcpyHostToDevice));
            k_dom<<<(W + WPB - 1) / WPB, 256>>>(dc.masks, W, R, d_out, cap, dc.counter, dom_static, dom_chunk, d_ret);
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());
            std::vector<uint32_t> h(dwords), ret(max_id);
            uint32_t counter = 0;
            HIP_OK(hipMemcpy(h.data(), d_out, dwords * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(ret.data(), d_ret, (size_t)max_id * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(&counter, dc.counter, 4, hipMemcpyDeviceToHost));
            HIP_OK(hipFree(d_out));
            Check ck;
            verify(model, max_id, cap, alloc, counter, [&](uint32_t s) -> Cell {
                const uint32_t v = h[dom_plane_index(s, 0)];
                if (v == POISON) return Cell{Cell::POISONED, 0};
                if (v == 0xFFFFFFFFu) return Cell{Cell::SENTINEL, 0};
                return Cell{Cell::ENTRY, v};
            }, ck);
            // 5: only plane 0 is the writer's; the returned slots
            for (uint32_t s = 0; s < alloc && ck.err.empty(); ++s)
                for (uint32_t pl = 1; pl < DOM_PLANES; ++pl)
                    if (h[dom_plane_index(s, pl)] != POISON) { ck.fail("plane %llu of slot %llu was written", pl, s); break; }
            for (uint32_t w = 0; w < W && ck.err.empty(); ++w)
                for (uint32_t r = 0; r < R && ck.err.empty(); ++r)
                    for (uint32_t l = 0; l < 64; ++l) {
                        const uint32_t id = entry_id(w, R, r, l), got = ret[id - 1];
                        const bool emit = (mk.at(w, r) >> l) & 1;
                        const uint32_t want = emit ? ck.slot_of_id[id] : NONE;   // NONE: the entry's slot is >= capacity
                        if (got != want) { ck.fail("entry %llu: reserve returned %llu, expected %llu", id, got, want); break; }
                    }
            report(name, W, cap, counter, ck);
            if (ci == 0) for (uint32_t c : capacities(model, ck, total)) caps.push_back(c);
        }
        HIP_OK(hipFree(d_ret));
        dc.release();
    }
}

template <class T, uint32_t CHUNK>
static void run_chunk(const std::string& name, uint64_t seed) {
    run_flat<T>(name, seed, MaskPlan{0, {CHUNK}, {0}}, 64, [](const Masks& mk) { return model_chunk(mk, CHUNK); },
                [](const uint64_t* m, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter) {
                    k_chunk<T, CHUNK><<<(W + WPB - 1) / WPB, 256>>>(m, W, R, out, cap, counter, Val<T>::sentinel());
                });
}
template <class T, uint32_t CAP>
static void run_buffered(const std::string& name, uint64_t seed) {
    // full rounds in front of the fills: five departures put a wave into the 256-slot regime, seventeen into the 2048-slot one (CAP = 64: a
    // full round sends the stage of the round before; CAP < 64: every full round leaves directly)
    const uint32_t p1 = CAP >= 64 ? 5 : 4, p2 = CAP >= 64 ? 17 : 16;
    run_flat<T>(name, seed, MaskPlan{CAP, {256, 2048}, {p1, p2}}, 96, [](const Masks& mk) { return model_buffered(mk, CAP); },
                [](const uint64_t* m, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter) {
                    k_buffered<T, CAP><<<(W + WPB - 1) / WPB, 256>>>(m, W, R, out, cap, counter);
                });
}
template <class T, uint32_t CAP>
static void run_staged(const std::string& name, uint64_t seed, uint32_t chunk) {
    run_flat<T>(name, seed, MaskPlan{CAP, {std::max(64u, chunk)}, {0}}, 64, [chunk](const Masks& mk) { return model_staged(mk, CAP, chunk); },
                [chunk](const uint64_t* m, uint32_t W, uint32_t R, T* out, uint32_t cap, uint32_t* counter) {
                    k_staged<T, CAP><<<(W + WPB - 1) / WPB, 256>>>(m, W, R, out, cap, counter, Val<T>::sentinel(), chunk);
                });
}

int main() {
    printf("STAGES CAND_STAGE=%u RARE_STAGE=%u\n", CAND_STAGE, RARE_STAGE);
    run_chunk<Hit, HIT_CHUNK>("ChunkWriter<Hit,HIT_CHUNK>", 0x5EED0100);
    run_chunk<Candidate, CAND_CHUNK>("ChunkWriter<Candidate,CAND_CHUNK>", 0x5EED0200);
    run_buffered<Candidate, 64>("BufferedWriter<Candidate>", 0x5EED0300);
    run_buffered<RareAnchor, 64>("BufferedWriter<RareAnchor>", 0x5EED0400);
    run_buffered<uint32_t, 64>("BufferedWriter<uint32_t>", 0x5EED0500);
    run_buffered<uint2, RARE_STAGE>("BufferedWriter<uint2,RARE_STAGE>", 0x5EED0600);
    run_staged<Candidate, CAND_STAGE>("StagedChunkWriter<Candidate,CAND_STAGE>/64", 0x5EED0700, 64);
    run_staged<Candidate, CAND_STAGE>("StagedChunkWriter<Candidate,CAND_STAGE>/1024", 0x5EED0800, 1024);
    run_dom("DomWriter/static/256", ANCHOR_CHUNK, 256);
    run_dom("DomWriter/static/1024", ANCHOR_CHUNK, ANCHOR_CHUNK);
    run_dom("DomWriter/reserved/256", 0, 256);
    run_dom("DomWriter/reserved/1024", 0, ANCHOR_CHUNK);
    printf("DONE cases=%d failed=%d\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
