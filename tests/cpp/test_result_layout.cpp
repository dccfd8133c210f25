// Host-only: the byte layout of the result blocks (csrc/result_layout.h) against the formulas the scanner has always allocated and
// pointed with, written out here. Built with g++ -fsanitize=address,undefined by tests/test_result_layout_host.py.
#include <cstddef>
#include <cstdio>

#include "result_layout.h"

static int failures = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) { ++failures; std::printf("FAIL line %d (recs %zu, ids %zu): %s\n", __LINE__, recs, ids, #cond); } \
    } while (0)

int main() {
    const size_t caps[] = {0, 1, 2, 3, 7, 8, 1000, 65537};
    for (size_t recs : caps) {
        for (size_t ids : caps) {
            const mxy::ResultLayout l{recs, ids};
            CHECK(l.ids_offset() == recs * 16);
            CHECK(l.offs_offset() % 8 == 0);
            CHECK(l.offs_offset() >= l.ids_offset() + 4 * ids);
            CHECK(l.offs_offset() + 8 * ids <= l.bytes());
            // the pinned mirror: what it is allocated with, and where the kernels' parameters point
            CHECK(l.bytes() == recs * 16 + ids * 12 + 64);
            CHECK(l.offs_offset() == recs * 16 + ((ids * 4 + 7) & ~(size_t)7));
            // the block of the copy path, laid out for the counts of the scan: hb | ib | ob
            const size_t hb = recs * 16, ib = ((ids * 4) + 7) & ~(size_t)7, ob = ids * 8;
            CHECK(l.ids_offset() == hb);
            CHECK(l.offs_offset() == hb + ib);
            CHECK(l.end() == hb + ib + ob);
            CHECK(l.end() <= l.bytes());
        }
    }
    if (failures) return 1;
    std::printf("result layout: ok\n");
    return 0;
}
