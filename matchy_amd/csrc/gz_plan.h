// Host plan of a gz scan (inflate.h): where the DEFLATE body of every gzip file of a pack lies, where its text goes in the batch, and
// in which order the waves of k_gz_inflate take the files. Host only (no HIP include) and header-only, like input_packer.h: the unit
// test builds this file with nothing else.
//
// Layout: the members lie end to end in table order, one '\n' — the separator, not the input's — behind every non-empty member:
// start[0] = 0, start[i + 1] = start[i] + cap[i] + 1 for cap[i] != 0 and start[i] otherwise. Segment i of the scan is member i; a member
// whose header does not parse has capacity 0 and keeps its index.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace mxy {

// bit-identical to matchy_gz_member_t: a whole gzip file at packed[offset, offset + len); out_len 0 = take ISIZE from its last four bytes
struct GzMemberIn { uint64_t offset; uint32_t len, out_len; };

// status values the plan itself gives out (inflate_core.h has them all)
constexpr int32_t GZ_PLAN_OK = 0, GZ_PLAN_BAD_HEADER = 1, GZ_PLAN_TRUNCATED = 2;

// body: offset in `packed` of the first DEFLATE byte; body_len: bytes from there to the member's end, the trailer included.
// start / cap: where the text goes in the batch, and how many bytes of it there may be.
struct GzPlanned { uint64_t body; uint32_t body_len, start, cap; int32_t status; };

struct GzPlan {
    std::vector<GzPlanned> members;
    std::vector<uint32_t> starts;   // one per member: the segment table of the scan
    std::vector<uint32_t> order;    // the members the device inflates (status OK so far), largest capacity first, ties in table order
    uint64_t total = 0;             // bytes of the batch
    uint64_t packed_bytes = 0;      // compressed bytes of all members
};

// RFC 1952 header of the file p[0, len): magic, CM = 8, no reserved FLG bit; FEXTRA, FNAME, FCOMMENT and FHCRC are skipped. Positions are
// 64-bit throughout, so no field of the file can wrap one. `body` = offset of the first DEFLATE byte.
inline int32_t gz_parse_header(const uint8_t* p, uint64_t len, uint64_t& body) {
    body = 0;
    if (len < 10 || p[0] != 0x1F || p[1] != 0x8B || p[2] != 8) return GZ_PLAN_BAD_HEADER;
    const uint8_t flg = p[3];
    if (flg & 0xE0) return GZ_PLAN_BAD_HEADER;
    uint64_t pos = 10;
    if (flg & 4) {   // FEXTRA
        if (len - pos < 2) return GZ_PLAN_BAD_HEADER;
        const uint64_t xlen = (uint64_t)p[pos] | (uint64_t)p[pos + 1] << 8;
        pos += 2;
        if (len - pos < xlen) return GZ_PLAN_BAD_HEADER;
        pos += xlen;
    }
    for (const uint8_t bit : {(uint8_t)8, (uint8_t)16}) {   // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        while (pos < len && p[pos] != 0) ++pos;
        if (pos >= len) return GZ_PLAN_BAD_HEADER;
        ++pos;
    }
    if (flg & 2) {   // FHCRC
        if (len - pos < 2) return GZ_PLAN_BAD_HEADER;
        pos += 2;
    }
    body = pos;
    return GZ_PLAN_OK;
}

// False with `err` set: nothing to scan (n == 0), a member outside packed[0, packed_len), or a batch of 2^31 bytes or more.
inline bool gz_plan(const uint8_t* packed, uint64_t packed_len, const GzMemberIn* in, size_t n, GzPlan& plan, std::string& err) {
    plan = GzPlan();
    if (!in || n == 0) { err = "gz plan: no members"; return false; }
    if (n > 0x7FFFFFFFull) { err = "gz plan: too many members"; return false; }
    plan.members.resize(n);
    plan.starts.resize(n);
    uint64_t start = 0;
    for (size_t i = 0; i < n; ++i) {
        const GzMemberIn& m = in[i];
        if (m.offset > packed_len || m.len > packed_len - m.offset) { err = "gz plan: member " + std::to_string(i) + " lies outside the buffer"; return false; }
        GzPlanned& g = plan.members[i];
        const uint8_t* p = packed + m.offset;
        uint64_t body = 0;
        g.status = gz_parse_header(p, m.len, body);
        if (g.status == GZ_PLAN_OK && m.len - body < 8) g.status = GZ_PLAN_TRUNCATED;   // no room for the trailer
        g.body = m.offset + body;
        g.body_len = g.status == GZ_PLAN_OK ? (uint32_t)(m.len - body) : 0u;
        g.cap = 0;
        if (g.status == GZ_PLAN_OK) {
            const uint8_t* t = p + m.len - 4;
            g.cap = m.out_len ? m.out_len : (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        }
        if (start + g.cap + 1 >= (1ull << 31)) { err = "gz plan: the inflated batch reaches 2^31 bytes at member " + std::to_string(i); return false; }
        g.start = (uint32_t)start;
        plan.starts[i] = g.start;
        if (g.cap) start += (uint64_t)g.cap + 1;
        plan.packed_bytes += m.len;
    }
    plan.total = start;
    for (size_t i = 0; i < n; ++i) if (plan.members[i].status == GZ_PLAN_OK) plan.order.push_back((uint32_t)i);
    std::stable_sort(plan.order.begin(), plan.order.end(), [&](uint32_t a, uint32_t b) { return plan.members[a].cap > plan.members[b].cap; });
    return true;
}

}  // namespace mxy
