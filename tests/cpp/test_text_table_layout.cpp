// text_table.h and lds_aggregator.h alone: the layout the host and the kernels of the device text table share (slot words, hash
// masking, home slot, text word, pool padding, table size, counter lines) and the home slot and LDS size of the aggregator, on the host.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I matchy_amd/csrc
//        tests/cpp/test_text_table_layout.cpp -o /tmp/test_text_table_layout      (no library: only the inline functions are used)
#include <cstdio>
#include <cstdlib>
#include <random>

#include "lds_aggregator.h"
#include "text_table.h"

using namespace mxy;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    std::mt19937_64 rng(5);
    // hash masking: n bits keep n bits; 0 bits make every hash equal; 64 and more keep all
    CHECK(text_hash_mask(0) == 0 && text_hash_mask(4) == 15 && text_hash_mask(63) == (~0ull >> 1));
    CHECK(text_hash_mask(64) == ~0ull && text_hash_mask(65) == ~0ull && text_hash_mask(1000) == ~0ull);
    // home slot: inside the table, and the high half of the hash counts
    for (uint32_t bits = 4; bits <= 31; ++bits) {
        const uint32_t mask = (1u << bits) - 1;
        for (int it = 0; it < 1000; ++it) CHECK(text_home(rng(), mask) <= mask);
    }
    CHECK(text_home(0x0000000100000000ull, 0xFFFF) != text_home(0, 0xFFFF));
    // text word and pool padding
    for (unsigned long long off : {0ull, 8ull, (1ull << 32) + 8, (1ull << 40) - 8})
        for (uint32_t len : {0u, 1u, 7u, 8u, 253u, 0xFFFFFFu}) {
            const unsigned long long w = text_word(off, len);
            CHECK(text_word_off(w) == off && text_word_len(w) == len);
        }
    for (uint32_t len = 0; len < 100; ++len) {
        const unsigned long long b = text_pool_bytes(len);
        CHECK(b >= len && b < (unsigned long long)len + TEXT_POOL_ALIGN && b % TEXT_POOL_ALIGN == 0);
    }
    CHECK(text_pool_bytes(0xFFFFFFu) == 0x1000000ull);
    // table size: a power of two, at least the floor, at most half full
    for (unsigned long long entries : {0ull, 1ull, 7ull, 8ull, 9ull, 32768ull, 32769ull, 1ull << 29, (1ull << 30)})
        for (unsigned long long floor_slots : {0ull, 1ull, 64ull, 65ull, 1ull << 16}) {
            const unsigned long long s = text_slots_for(entries, floor_slots);
            CHECK((s & (s - 1)) == 0 && s >= 16 && s >= floor_slots && s >= 2 * entries);
            CHECK(s == 16 || s / 2 < floor_slots || s / 2 < 2 * entries);
        }
    static_assert(sizeof(TextCounters) == 256 && offsetof(TextCounters, n_counted) == 128 && offsetof(TextCounters, n_new) == 136, "two 128-byte counter lines");
    static_assert(offsetof(TextSlot, aux) == 24, "the owner's word (the tally's count) is the last word of the slot");
    // published: bit 63 and not the owner's empty word, for both empty words
    CHECK(text_is_published(TEXT_PUBLISHED, ~0ull) && text_is_published(TEXT_PUBLISHED | 7, 0) && !text_is_published(~0ull, ~0ull) && !text_is_published(0, 0));
    CHECK(!text_is_published(12345, 0) && !text_is_published(12345, ~0ull));
    // the aggregators of k_tally_claim (8 bits, 4 probes, 1 leader round) and of the segment passes (7, 4, 4)
    using TallyAgg = LdsAggregator<8, 4, 1>;
    using SegAgg = LdsAggregator<7, 4, 4>;
    static_assert(TallyAgg::SLOTS == 256 && TallyAgg::LDS_BYTES == 2 * sizeof(uint32_t) * TallyAgg::SLOTS, "a key word and a count word per entry");
    static_assert(2 * sizeof(uint32_t) * TallyAgg::SLOTS <= 2 * 1280, "the aggregator fits two LDS granules");
    static_assert(SegAgg::SLOTS == 128 && SegAgg::LDS_BYTES <= 1280, "the segment aggregator fits one LDS granule");
    for (uint32_t s : {0u, 1u, 255u, 256u, 0x7FFFFFFFu, 0xFFFFFFFEu}) CHECK(TallyAgg::home(s) < TallyAgg::SLOTS && SegAgg::home(s) < SegAgg::SLOTS);
    printf("text table layout: ok\n");
    return 0;
}
