// distinct.h alone: what is the distinct-text set's own of the layout the host and its kernels share (order key, type rank), on the
// host. The table's layout is in test_text_table_layout.cpp.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I matchy_amd/csrc
//        tests/cpp/test_distinct_layout.cpp -o /tmp/test_distinct_layout      (no library: only the inline functions are used)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>

#include "distinct.h"

using namespace mxy;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    // states of the order word: a key never looks like one of the other two, whatever its fields
    const uint32_t max_start = DISTINCT_MAX_LEN - 1, max_index = DISTINCT_MAX_INDEX - 1;
    CHECK(!distinct_is_key(DISTINCT_EMPTY) && !distinct_is_key(DISTINCT_PUBLISHED) && DISTINCT_EMPTY != DISTINCT_PUBLISHED);
    for (uint32_t t = 0; t < 16; ++t) {
        const unsigned long long k = distinct_order_key(max_start, t, max_index);
        CHECK(distinct_is_key(k) && distinct_key_index(k) == max_index && (k >> (DISTINCT_RANK_BITS + DISTINCT_INDEX_BITS)) == max_start);
    }
    CHECK(distinct_order_key(0, IT_IPV6, 0) == 0);
    // type rank: the chunk-path extractor order, hashes share a rank, unknown types sort last and still fit the field
    const uint32_t order[] = {IT_IPV6, IT_IPV4, IT_EMAIL, IT_DOMAIN, IT_MD5, IT_BITCOIN, IT_ETHEREUM, IT_MONERO};
    for (uint32_t i = 0; i < 8; ++i) CHECK(distinct_type_rank(order[i]) == i);
    for (uint32_t t : {IT_SHA1, IT_SHA256, IT_SHA384, IT_SHA512}) CHECK(distinct_type_rank(t) == 4);
    CHECK(distinct_type_rank(200) == 8 && distinct_type_rank(200) < (1u << DISTINCT_RANK_BITS));
    // keys order like (start, rank, index) tuples
    std::mt19937_64 rng(5);
    const uint32_t types[] = {IT_DOMAIN, IT_EMAIL, IT_IPV4, IT_IPV6, IT_MD5, IT_SHA512, IT_BITCOIN, IT_ETHEREUM, IT_MONERO};
    for (int it = 0; it < 200000; ++it) {
        // half of the draws from a handful of values, so that ties in the leading fields are common
        auto draw = [&](uint32_t max) { return (rng() & 1) ? (uint32_t)(rng() % 3) * (max / 2) : (uint32_t)(rng() % ((unsigned long long)max + 1)); };
        const uint32_t s1 = draw(max_start), s2 = draw(max_start), i1 = draw(max_index), i2 = draw(max_index);
        const uint32_t t1 = types[rng() % 9], t2 = types[rng() % 9];
        const auto a = std::make_tuple(s1, distinct_type_rank(t1), i1), b = std::make_tuple(s2, distinct_type_rank(t2), i2);
        const unsigned long long ka = distinct_order_key(s1, t1, i1), kb = distinct_order_key(s2, t2, i2);
        CHECK((a < b) == (ka < kb) && (a == b) == (ka == kb));
        CHECK(distinct_key_index(ka) == i1);
    }
    printf("distinct layout: ok\n");
    return 0;
}
