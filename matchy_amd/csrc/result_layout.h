// Byte layout of the host blocks the final records of a scan come back in: records, the pattern ids of their glob results, the data
// offsets of those ids, in one pinned block. Plain arithmetic (tests/cpp/test_result_layout.cpp runs it on the host).
#pragma once
#include <cstddef>

namespace mxy {

//   FinalHit[recs_cap] | u32 ids[ids_cap] | pad to 8 | i64 offs[ids_cap]
// The pinned mirror the lookup kernels write is laid out for its capacities and allocated with bytes(); the block of the copy path is
// laid out for the counts of the scan and is end() bytes long.
struct ResultLayout {
    static constexpr size_t REC_BYTES = 16;   // sizeof(FinalHit)
    size_t recs_cap = 0, ids_cap = 0;
    size_t ids_offset() const { return recs_cap * REC_BYTES; }
    size_t offs_offset() const { return ids_offset() + ((ids_cap * 4 + 7) & ~(size_t)7); }
    size_t end() const { return offs_offset() + ids_cap * 8; }
    size_t bytes() const { return recs_cap * REC_BYTES + ids_cap * 12 + 64; }   // end() and slack
};

}  // namespace mxy
