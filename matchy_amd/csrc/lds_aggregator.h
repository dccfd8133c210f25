// Counting into a few hot global words without putting every wave on one counter line: lanes of a wave with the same key add once
// (a bounded number of leader rounds), the adds go to a small per-workgroup open-addressing table key -> count in LDS, and one global
// add per occupied entry flushes it when the workgroup ends. Used by k_tally_claim (tally.hip: key = table slot) and by k_seg_records /
// k_seg_lines (segments.hip: key = segment). No lane waits for another and every loop has a fixed bound.
#pragma once
#include <cstdint>

#include "hashes.h"

namespace mxy {

// BITS: 2^BITS entries of a key word and a count word; PROBES: entries a key tries before it gives up; ROUNDS: leader rounds per wave.
// The workgroup owns `keys` and `counts` (SLOTS words each, in LDS); NO_KEY never is a key.
template <uint32_t BITS, uint32_t PROBES, uint32_t ROUNDS>
struct LdsAggregator {
    static constexpr uint32_t SLOTS = 1u << BITS, NO_KEY = 0xFFFFFFFFu;
    static constexpr uint32_t LDS_BYTES = 2 * SLOTS * (uint32_t)sizeof(uint32_t);
    static MXY_HD uint32_t home(uint32_t key) { return (key * 2654435761u) >> (32 - BITS); }

#if defined(__HIPCC__)
    // every thread of the workgroup (`threads` of them), in front of a __syncthreads()
    static __device__ __forceinline__ void clear(uint32_t* keys, uint32_t* counts, uint32_t threads) {
        for (uint32_t e = threadIdx.x; e < SLOTS; e += threads) { keys[e] = NO_KEY; counts[e] = 0; }
    }
    // `amount` for `key`; false when the key found no room within PROBES probes: the caller adds to the global word itself
    static __device__ __forceinline__ bool add(uint32_t* keys, uint32_t* counts, uint32_t key, uint32_t amount) {
        uint32_t h = home(key);
#pragma unroll
        for (uint32_t t = 0; t < PROBES; ++t, h = (h + 1u) & (SLOTS - 1u)) {
            uint32_t k = keys[h];
            if (k == NO_KEY) k = atomicCAS(&keys[h], NO_KEY, key);
            if (k == NO_KEY || k == key) { atomicAdd(&counts[h], amount); return true; }
        }
        return false;
    }
    // One count for `key` of every lane in `counting` (a ballot). Every lane of the wave calls this: the leader rounds are wave-wide. In
    // each round the lanes that share the key of the first lane still uncounted are taken over by that lane; what is left after the
    // rounds counts for itself. Then every lane that has something to add does so, once, in one pass over the aggregator. Returns
    // what the lane's add amounted to when it found no room (the caller adds that to the global word of `key`), else 0.
    static __device__ __forceinline__ uint32_t count(uint32_t* keys, uint32_t* counts, unsigned long long counting, uint32_t key, uint32_t lane) {
        uint32_t amount = (uint32_t)(counting >> lane) & 1u;   // what this lane adds for `key`: its own count until a leader takes it over
        unsigned long long left = counting;
#pragma unroll
        for (uint32_t r = 0; r < ROUNDS; ++r) {
            if (!left) break;
            const uint32_t first = (uint32_t)__ffsll((long long)left) - 1u;
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)first);
            // all lanes of a key leave in one round, so a lane that is still in `left` has amount 1 and a leader never matches again
            const unsigned long long same = __ballot(((left >> lane) & 1ull) && key == lead);
            if ((same >> lane) & 1ull) amount = lane == first ? (uint32_t)__popcll(same) : 0u;
            left &= ~same;
        }
        return amount && !add(keys, counts, key, amount) ? amount : 0u;
    }
    // every thread of the workgroup, behind a __syncthreads(): flush_one(key, count) for every occupied entry (it tests the key's bound)
    template <class F>
    static __device__ __forceinline__ void flush(const uint32_t* keys, const uint32_t* counts, uint32_t threads, F flush_one) {
        for (uint32_t e = threadIdx.x; e < SLOTS; e += threads) {
            const uint32_t k = keys[e], c = counts[e];
            if (k != NO_KEY && c) flush_one(k, c);
        }
    }
#endif
};

}  // namespace mxy
