// tally.h alone: what the host and the kernels of the hit tally share (slot states, compact-record length, type-seeded hash) and the
// host's read-out logic (entry order, selection for a top-N, merge of several workers' exports), on the host.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I matchy_amd/csrc
//        tests/cpp/test_tally_layout.cpp -o /tmp/test_tally_layout      (no library: only the inline functions are used)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tally.h"

using namespace mxy;

#define MD5_TEXT "9e107d9d372bb6826bd81d3542a419d6"
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static TallyEntry entry(const char* text, uint8_t type, uint64_t count) { TallyEntry e; e.text = text; e.item_type = type; e.count = count; return e; }

int main() {
    // slot states: empty is all-zero bytes, a claim word never looks published, a published word carries the type
    CHECK(TALLY_EMPTY == 0 && !tally_is_published(TALLY_EMPTY));
    for (uint32_t idx : {0u, 1u, 12345u, 0xFFFFFFEFu}) {
        const unsigned long long w = tally_claim_word(idx);
        CHECK(w != TALLY_EMPTY && !tally_is_published(w) && tally_claim_index(w) == idx && (w >> 32) <= 1);
    }
    CHECK(TALLY_MAX_RECORDS < (1ull << 32) - 1);   // index + 1 of every record fits 32 bits
    for (uint32_t t = 0; t < IT_COUNT; ++t) {
        const unsigned long long w = tally_published(t);
        CHECK(tally_is_published(w) && tally_state_type(w) == t && w != TALLY_EMPTY);
    }

    // compact-record length: c4_pack stores length - 7 in four bits; every length an IPv4 text can have comes back
    for (uint32_t len = 7; len <= 15; ++len)
        for (uint32_t data_off : {0u, 1u, (1u << C4_DATA_BITS) - 1})
            for (uint32_t prefix : {0u, 24u, 32u}) {
                const uint2 c = c4_pack(1000, len, data_off, prefix);
                CHECK(tally_c4_len(c.y) == len && c.x == 1000);
            }
    // usable: the text must lie inside the batch
    CHECK(tally_usable(0, 7, 7) && tally_usable(93, 7, 100) && !tally_usable(94, 7, 100) && !tally_usable(100, 0, 100) && !tally_usable(0xFFFFFFFFu, 7, 100));
    CHECK(tally_usable(5, 0xFFFFFFu, 0x7FFF0000u) && !tally_usable(0x7FFEFFFFu, 0xFFFFFFu, 0x7FFF0000u));

    // the hash is seeded with the type: same bytes, other type, other hash; masking keeps the low bits; 0 bits collide everything
    const uint8_t text[] = "9e107d9d372bb6826bd81d3542a419d6";
    const unsigned long long all = text_hash_mask(64);
    CHECK(tally_hash(text, 32, IT_MD5, all) == xxh64(text, 32, IT_MD5));
    CHECK(tally_hash(text, 32, IT_MD5, all) != tally_hash(text, 32, IT_DOMAIN, all));
    CHECK(tally_hash(text, 32, IT_DOMAIN, all) == xxh64(text, 32, 0));
    CHECK(tally_hash(text, 31, IT_MD5, all) != tally_hash(text, 32, IT_MD5, all));
    CHECK(tally_hash(text, 32, IT_MD5, text_hash_mask(4)) == (xxh64(text, 32, IT_MD5) & 15));
    for (uint32_t t = 0; t < IT_COUNT; ++t) CHECK(tally_hash(text, 32, t, text_hash_mask(0)) == 0);

    // read-out order: count descending, extractor order of the type, text bytewise ascending (a prefix first, bytes unsigned)
    {
        std::vector<TallyEntry> v = {
            entry("b.example.com", IT_DOMAIN, 5), entry("a.example.com", IT_DOMAIN, 5), entry("a.example.co", IT_DOMAIN, 5), entry("10.0.0.1", IT_IPV4, 5),
            entry("2001:db8::1", IT_IPV6, 5), entry("zzz", IT_DOMAIN, 9), entry("x@y.com", IT_EMAIL, 5), entry(MD5_TEXT, IT_MD5, 5),
            entry("A.example.com", IT_DOMAIN, 5), entry("\xC3\xA9.example.com", IT_DOMAIN, 5), entry("10.0.0.1", IT_IPV4, 1),
            entry("aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", IT_SHA1, 5), entry("1BoatSLRHtKNngkdXEeobR76b53LETtpyT", IT_BITCOIN, 5),
        };
        std::vector<TallyEntry> w = v;
        tally_order(w, 0);
        const char* want[] = {"zzz", "2001:db8::1", "10.0.0.1", "x@y.com", "A.example.com", "a.example.co", "a.example.com", "b.example.com",
                              "\xC3\xA9.example.com", MD5_TEXT, "aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", "1BoatSLRHtKNngkdXEeobR76b53LETtpyT", "10.0.0.1"};
        CHECK(w.size() == 13);
        for (size_t i = 0; i < w.size(); ++i) CHECK(w[i].text == want[i]);
        CHECK(w.back().count == 1);
        // a total order: no two different entries tie, whatever the input order
        for (size_t i = 0; i + 1 < w.size(); ++i) CHECK(tally_entry_less(w[i], w[i + 1]) && !tally_entry_less(w[i + 1], w[i]));
        std::mt19937 rng(7);
        for (int it = 0; it < 50; ++it) {
            std::vector<TallyEntry> s = v;
            std::shuffle(s.begin(), s.end(), rng);
            tally_order(s, 4);
            CHECK(s.size() == 4);
            for (size_t i = 0; i < 4; ++i) CHECK(s[i].text == want[i]);
        }
        // hash types share a rank: equal text cannot happen across them (other lengths), equal count and rank fall to the text
        CHECK(tally_entry_less(entry("aa", IT_MD5, 1), entry("ab", IT_SHA512, 1)) && tally_entry_less(entry("aa", IT_SHA512, 1), entry("ab", IT_MD5, 1)));
        CHECK(tally_entry_less(entry("aa", IT_MD5, 1), entry("aa", IT_SHA1, 1)) && !tally_entry_less(entry("aa", IT_SHA1, 1), entry("aa", IT_MD5, 1)));
    }

    // selection for a top-N from the export alone: everything in front of the cut by (count, rank) and the whole group tied with it
    {
        std::vector<TallyExport> ex;
        auto add = [&](uint64_t count, uint32_t type) { TallyExport x{}; x.count = count; x.item_type = type; x.slot = (uint32_t)ex.size(); x.text = text_word(8 * ex.size(), 5); ex.push_back(x); };
        add(1, IT_IPV4); add(7, IT_DOMAIN); add(1, IT_IPV4); add(3, IT_IPV4); add(1, IT_DOMAIN); add(3, IT_IPV6); add(1, IT_IPV4); add(7, IT_IPV4);
        auto sel = [&](size_t limit) { std::vector<uint32_t> s = tally_select(ex, limit); return std::set<uint32_t>(s.begin(), s.end()); };
        CHECK(sel(0).size() == 8 && sel(8).size() == 8 && sel(100).size() == 8);
        CHECK((sel(1) == std::set<uint32_t>{7}));                 // 7 x IPv4 is in front of 7 x Domain
        CHECK((sel(2) == std::set<uint32_t>{1, 7}));
        CHECK((sel(3) == std::set<uint32_t>{1, 7, 5}));           // 3 x IPv6 before 3 x IPv4
        CHECK((sel(4) == std::set<uint32_t>{1, 7, 5, 3}));
        CHECK((sel(5) == std::set<uint32_t>{1, 7, 5, 3, 0, 2, 6}));   // the cut falls into the three 1 x IPv4: all of them, the texts decide
        CHECK((sel(6) == sel(5) && sel(7) == sel(5)));
        std::vector<TallyExport> none;
        CHECK(tally_select(none, 3).empty());
    }

    // merge of several workers' exports: counts of equal (type, text) add up, the same text under another type stays apart
    {
        std::vector<std::vector<TallyEntry>> parts = {
            {entry("10.0.0.1", IT_IPV4, 5), entry("a.example.com", IT_DOMAIN, 2), entry("abc", IT_MD5, 1)},
            {},
            {entry("a.example.com", IT_DOMAIN, 3), entry("10.0.0.1", IT_IPV4, 1), entry("abc", IT_SHA1, 1), entry("b.example.com", IT_DOMAIN, 6)},
            {entry("10.0.0.1", IT_IPV4, 1)},
        };
        std::vector<TallyEntry> m = tally_merge(parts);
        CHECK(m.size() == 5);
        tally_order(m, 0);
        CHECK(m[0].text == "10.0.0.1" && m[0].count == 7 && m[0].item_type == IT_IPV4);
        CHECK(m[1].text == "b.example.com" && m[1].count == 6);
        CHECK(m[2].text == "a.example.com" && m[2].count == 5);
        CHECK(m[3].text == "abc" && m[3].item_type == IT_MD5 && m[3].count == 1);
        CHECK(m[4].text == "abc" && m[4].item_type == IT_SHA1 && m[4].count == 1);
        std::vector<TallyEntry> cut = tally_merge(parts);
        tally_order(cut, 2);
        CHECK(cut.size() == 2 && cut[1].text == "b.example.com");
        uint64_t sum = 0;
        for (const TallyEntry& e : m) sum += e.count;
        CHECK(sum == 20);
        CHECK(tally_merge({}).empty());
    }
    printf("tally layout: ok\n");
    return 0;
}
