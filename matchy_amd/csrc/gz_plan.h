// Host plan of a gz scan (inflate.h): where the DEFLATE body of every gzip file of a pack lies, where its text goes in the batch, and
// in which order the waves of k_gz_inflate take the files. Host only (no HIP include) and header-only, like input_packer.h: the unit
// test builds this file with nothing else.
//
// Layout: the members lie end to end in table order, one '\n' — the separator, not the input's — behind every non-empty member:
// start[0] = 0, start[i + 1] = start[i] + cap[i] + 1 for cap[i] != 0 and start[i] otherwise. Segment i of the scan is member i; a member
// whose header does not parse has capacity 0 and keeps its index.
//
// Multi-member files (gz_split_members, gz_plan_files, below): the members of a file are found on the host, laid out as ONE segment and
// inflated by one wave each.
//
// Windows (gz_next_window, gz_plan_window, below): a file larger than a batch is walked window by window — runs of whole members — and
// every window is planned like a file, with the carry of the window in front laid in front of its text.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
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
// 64-bit throughout, so no field of the file can wrap one. `body` = offset of the first DEFLATE byte. max_str: the most bytes FNAME and
// FCOMMENT may have each, the NUL included; a longer one does not parse (the member split bounds what one candidate header can cost).
inline int32_t gz_parse_header(const uint8_t* p, uint64_t len, uint64_t& body, uint64_t max_str = ~0ull) {
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
        const uint64_t room = std::min(len - pos, max_str);
        const void* nul = room ? memchr(p + pos, 0, room) : nullptr;
        if (!nul) return GZ_PLAN_BAD_HEADER;
        pos = (uint64_t)((const uint8_t*)nul - p) + 1;
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

// ------------------------------------------------------------------------------------------------ multi-member files
// A gzip file is a sequence of members (RFC 1952), each an independent DEFLATE stream: a file of k members can be inflated by k waves.
// The host only GUESSES where the members start; the device verifies every guess with the rules it already has: a member must end
// exactly 8 bytes before its piece's end (otherwise TRUNCATED or TRAILING_DATA) and its CRC-32 and ISIZE must match. If every piece of a
// file is OK the pieces tile the file with complete valid members, which is what gzread would parse; a false cut cannot give all-OK pieces.

// bit-identical to matchy_gz_file_t: a whole gzip file, of one member or many, at packed[offset, offset + len)
struct GzFileIn { uint64_t offset, len; };

// BSIZE of a BGZF member (FEXTRA subfield 'B','C' with SLEN 2: the member's length - 1) whose header p[0, len) has parsed; false: none
inline bool gz_bgzf_bsize(const uint8_t* p, uint64_t len, uint32_t& bsize) {
    if (len < 12 || !(p[3] & 4)) return false;
    const uint64_t xlen = (uint64_t)p[10] | (uint64_t)p[11] << 8;
    if (len - 12 < xlen) return false;
    for (uint64_t at = 12, end = 12 + xlen; end - at >= 4;) {   // SI1 SI2 SLEN data
        const uint64_t slen = (uint64_t)p[at + 2] | (uint64_t)p[at + 3] << 8;
        if (end - at - 4 < slen) return false;
        if (p[at] == 'B' && p[at + 1] == 'C' && slen == 2) { bsize = (uint32_t)p[at + 4] | (uint32_t)p[at + 5] << 8; return true; }
        at += 4 + slen;
    }
    return false;
}

// Offsets where the members of the file p[0, len) start; the first is always 0. From one member to the next:
//   BGZF member    BSIZE gives the length: the next member starts at pos + BSIZE + 1 — a cut only if that leaves room for the smallest
//                  member in front of it, lies inside the file and a header parses there; otherwise this member keeps the rest.
//   any other      the next position from body + 10 on (the smallest stream is 2 bytes, the trailer 8) with 1f 8b 08, no reserved FLG
//                  bit, XFL 0, 2 or 4, and a header that parses.
// A header the split looks for — every one but the file's first — may have at most GZ_SPLIT_MAX_STR bytes of FNAME and of FCOMMENT each,
// the NUL included (a file name has at most 255): a candidate then costs a bounded number of bytes, and a hostile file of header patterns
// with the FNAME bit and no NUL behind them costs time linear in its length. A real member with a longer string is not found, its
// predecessor reports TRAILING_DATA and the file falls back, like one with an unusual XFL.
// Every cut lies at least 20 bytes behind the one in front of it, so there are at most len / 18 of them; every read is inside p[0, len).
constexpr uint64_t GZ_SPLIT_MAX_STR = 256;
// The ONE copy of the cut rule above: the member at `pos` of the file p[0, len), whose header of `body` bytes has parsed. True with
// the next member's position and the length of its header; false: this member keeps the rest of the file.
inline bool gz_next_member(const uint8_t* p, uint64_t len, uint64_t pos, uint64_t body, uint64_t& next, uint64_t& next_body) {
    static const uint8_t magic[3] = {0x1F, 0x8B, 8};
    uint32_t bsize = 0;
    if (gz_bgzf_bsize(p + pos, len - pos, bsize)) {
        next = pos + bsize + 1;
        return !((uint64_t)bsize + 1 < body + 10 || next >= len || gz_parse_header(p + next, len - next, next_body, GZ_SPLIT_MAX_STR) != GZ_PLAN_OK);
    }
    for (uint64_t q = pos + body + 10;; ++q) {
        const void* hit = q < len ? memmem(p + q, len - q, magic, 3) : nullptr;
        if (!hit) return false;
        q = (uint64_t)((const uint8_t*)hit - p);
        if (len - q < 10) return false;   // no later position has room for a header either
        if (!(p[q + 3] & 0xE0) && (p[q + 8] == 0 || p[q + 8] == 2 || p[q + 8] == 4) && gz_parse_header(p + q, len - q, next_body, GZ_SPLIT_MAX_STR) == GZ_PLAN_OK) { next = q; return true; }
    }
}
inline void gz_split_members(const uint8_t* p, uint64_t len, std::vector<uint64_t>& cuts) {
    cuts.clear();
    cuts.push_back(0);
    uint64_t pos = 0, body = 0;   // the member in hand and the length of its header
    if (gz_parse_header(p, len, body) != GZ_PLAN_OK) return;
    for (uint64_t next = 0, nb = 0; gz_next_member(p, len, pos, body, next, nb); pos = next, body = nb) cuts.push_back(next);
}

// Windows (gz_plan_window, below): a file too large for one batch is scanned as runs of consecutive whole members. The walker finds the
// next run without walking the whole file first: from `from` — 0, or the end of the window in front — it steps from member to member by
// gz_next_member, so the cuts it yields over a file are exactly those of gz_split_members, and stops in front of the member that would
// push the window past max_text inflated bytes (the sum of the ISIZE fields) or max_comp compressed bytes. False — no window: nothing
// is left (from >= len), or the next member alone breaks a bound: its header does not parse, it has no room for a trailer, or its
// compressed length or its ISIZE is above max_member, max_comp or max_text. All sums are 64-bit; every read is inside p[0, len). The
// member that ends a window is stepped over once more by the next call, so a file costs at most twice the walk of gz_split_members.
// cuts: where the window's members start, appended (nullptr: not wanted).
struct GzWindow { uint64_t end = 0, text = 0; uint32_t members = 0; };
inline bool gz_next_window(const uint8_t* p, uint64_t len, uint64_t from, uint64_t max_comp, uint64_t max_text, uint64_t max_member, GzWindow& out,
                           std::vector<uint64_t>* cuts = nullptr) {
    out = GzWindow();
    out.end = from;
    if (from >= len) return false;
    uint64_t pos = from, body = 0;
    if (gz_parse_header(p + pos, len - pos, body, from ? GZ_SPLIT_MAX_STR : ~0ull) != GZ_PLAN_OK) return false;
    for (;;) {
        uint64_t next = 0, nb = 0;
        const bool more = gz_next_member(p, len, pos, body, next, nb);
        const uint64_t end = more ? next : len, mlen = end - pos;
        if (mlen - body < 8 || mlen > max_member) break;   // no room for the trailer; too long for one wave
        const uint8_t* t = p + end - 4;
        const uint64_t isize = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        if (isize > max_member || out.text + isize > max_text || end - from > max_comp || out.members == 0x7FFFFFFFu) break;
        if (cuts) cuts->push_back(pos);
        out.end = end; out.text += isize; ++out.members;
        if (!more) break;
        pos = next; body = nb;
    }
    return out.members != 0;
}

// The plan of a pack of files. The members of a file lie end to end with NOTHING between them — a line may span two members, BGZF cuts
// at arbitrary bytes — and one separator '\n' follows every file whose members' capacities sum to more than 0. Segment i of the scan is
// FILE i: starts[i] is where its first member's text goes. Every capacity is the member's own ISIZE.
struct GzFilesPlan {
    std::vector<GzPlanned> members;        // of all files, in file order and stream order
    std::vector<uint32_t> member_file;     // one per member: its file
    std::vector<uint32_t> first_member;    // n_files + 1: the members of file f are [first_member[f], first_member[f + 1])
    std::vector<uint32_t> starts, caps;    // one per file: the segment table of the scan, and the sum of its members' capacities
    std::vector<uint32_t> order;           // as GzPlan::order, over the members of all files
    uint64_t total = 0, packed_bytes = 0;
};

// False with `err` set: nothing to scan, a file outside packed[0, packed_len) or of 4 GiB or more, or a batch of 2^31 bytes or more.
inline bool gz_plan_files(const uint8_t* packed, uint64_t packed_len, const GzFileIn* files, size_t n_files, GzFilesPlan& plan, std::string& err) {
    plan = GzFilesPlan();
    if (!files || n_files == 0) { err = "gz plan: no files"; return false; }
    if (n_files > 0x7FFFFFFFull) { err = "gz plan: too many files"; return false; }
    plan.starts.resize(n_files);
    plan.caps.resize(n_files);
    plan.first_member.resize(n_files + 1);
    std::vector<uint64_t> cuts;
    uint64_t start = 0;   // of the file; sums are 64-bit and tested after every member, so an ISIZE of 0xFFFFFFFF is refused, not wrapped
    for (size_t f = 0; f < n_files; ++f) {
        const GzFileIn& in = files[f];
        if (in.offset > packed_len || in.len > packed_len - in.offset) { err = "gz plan: file " + std::to_string(f) + " lies outside the buffer"; return false; }
        if (in.len > 0xFFFFFFFFull) { err = "gz plan: file " + std::to_string(f) + " has 4 GiB or more"; return false; }
        const uint8_t* p = packed + in.offset;
        gz_split_members(p, in.len, cuts);
        if (plan.members.size() + cuts.size() > 0x7FFFFFFFull) { err = "gz plan: too many members"; return false; }
        plan.first_member[f] = (uint32_t)plan.members.size();
        plan.starts[f] = (uint32_t)start;
        uint64_t cap_sum = 0;
        for (size_t k = 0; k < cuts.size(); ++k) {
            const uint64_t at = cuts[k], mlen = (k + 1 < cuts.size() ? cuts[k + 1] : in.len) - at;
            GzPlanned g;
            uint64_t body = 0;
            g.status = gz_parse_header(p + at, mlen, body);
            if (g.status == GZ_PLAN_OK && mlen - body < 8) g.status = GZ_PLAN_TRUNCATED;   // no room for the trailer
            g.body = in.offset + at + body;
            g.body_len = g.status == GZ_PLAN_OK ? (uint32_t)(mlen - body) : 0u;
            g.cap = 0;
            if (g.status == GZ_PLAN_OK) {
                const uint8_t* t = p + at + mlen - 4;
                g.cap = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            }
            if (start + cap_sum + g.cap + 1 >= (1ull << 31)) { err = "gz plan: the inflated batch reaches 2^31 bytes in file " + std::to_string(f); return false; }
            g.start = (uint32_t)(start + cap_sum);
            cap_sum += g.cap;
            plan.members.push_back(g);
            plan.member_file.push_back((uint32_t)f);
        }
        plan.caps[f] = (uint32_t)cap_sum;
        if (cap_sum) start += cap_sum + 1;
        plan.packed_bytes += in.len;
    }
    plan.first_member[n_files] = (uint32_t)plan.members.size();
    plan.total = start;
    for (size_t i = 0; i < plan.members.size(); ++i) if (plan.members[i].status == GZ_PLAN_OK) plan.order.push_back((uint32_t)i);
    std::stable_sort(plan.order.begin(), plan.order.end(), [&](uint32_t a, uint32_t b) { return plan.members[a].cap > plan.members[b].cap; });
    return true;
}

// The plan of one window: packed[0, packed_len) holds the window's whole members (split here once more, like a file of gz_plan_files),
// carry_len bytes — the partial line the window in front left behind — lie in front of their text:
//   [carry][member 0 text] ... [member m - 1 text][one '\n', only if the window is the file's LAST and carry + capacities > 0]
// The members' starts are shifted by carry_len; the window is segment 0 of the scan and starts at 0; caps[0] is the sum of the
// members' capacities, without the carry. Refused like a file: a batch that reaches 2^31 bytes, the carry counted in.
inline bool gz_plan_window(const uint8_t* packed, uint64_t packed_len, uint32_t carry_len, bool last, GzFilesPlan& plan, std::string& err) {
    const GzFileIn file{0, packed_len};
    if (!gz_plan_files(packed, packed_len, &file, 1, plan, err)) return false;
    const uint64_t text = (uint64_t)carry_len + plan.caps[0];
    if (text + 1 >= (1ull << 31)) { err = "gz plan: the inflated batch reaches 2^31 bytes with the carry of " + std::to_string(carry_len) + " bytes in front of the window"; return false; }
    for (GzPlanned& g : plan.members) g.start += carry_len;
    plan.total = text + (last && text ? 1 : 0);
    return true;
}

// ------------------------------------------------------------------------------------------------ pieces of one stream
// One large member inflated by many waves (inflate_pieces.hip). A member is split when pieces are on and its body has at least
// 2 * piece_bytes bytes: piece i of it are the compressed bytes [i * piece_bytes, (i + 1) * piece_bytes) of the body, the last one
// shorter. A split member needs 2 bytes of symbol scratch per byte of its capacity. GZ_PIECE_SCRATCH_MAX bounds the scratch of one scan:
// 4 GiB = 2 * 2^31 bytes. It follows from the batch bound: a batch holds less than 2^31 bytes of text, so a plan that gz_plan accepts
// never reaches it, and symbol positions fit 32 bits; it is tested here all the same, so that the rule holds for any table a caller of
// this function builds. (A lower bound was tried first: at 1 GiB the pack of 64 files of 16 MiB split only half of its members, and the
// other half set the time of the scan.) Members are taken in claim order, largest first; one that would push the scratch past the
// bound stays unsplit, and so does an empty one.
constexpr uint32_t GZ_PIECE_BYTES_MIN = 512, GZ_PIECE_BYTES_MAX = 1u << 20;
constexpr uint64_t GZ_PIECE_SCRATCH_MAX = 1ull << 32;
inline bool gz_piece_bytes_valid(uint32_t piece_bytes) {
    return piece_bytes >= GZ_PIECE_BYTES_MIN && piece_bytes <= GZ_PIECE_BYTES_MAX && (piece_bytes & (piece_bytes - 1)) == 0;
}
struct GzPiecePlan {
    std::vector<uint32_t> split;         // the split members, in table order
    std::vector<uint32_t> first_piece;   // n_members + 1: the pieces of member i are [first_piece[i], first_piece[i + 1])
    std::vector<uint32_t> sym_base;      // one per member: where its symbols begin in the scratch (16-bit units)
    uint64_t scratch_syms = 0;
};
// `order` (GzPlan::order) loses the members that are split: they are not k_gz_inflate's in the first launch.
inline void gz_plan_pieces(const std::vector<GzPlanned>& members, std::vector<uint32_t>& order, uint32_t piece_bytes, GzPiecePlan& pp) {
    const size_t n = members.size();
    pp = GzPiecePlan();
    pp.first_piece.assign(n + 1, 0);
    pp.sym_base.assign(n, 0);
    if (!gz_piece_bytes_valid(piece_bytes)) return;
    std::vector<uint8_t> is_split(n, 0);
    uint64_t bytes = 0, pieces = 0;
    for (const uint32_t mi : order) {
        const GzPlanned& g = members[mi];
        const uint64_t np = ((uint64_t)g.body_len + piece_bytes - 1) / piece_bytes;
        if (g.status != GZ_PLAN_OK || g.cap == 0 || g.body_len < 2ull * piece_bytes || bytes + 2ull * g.cap > GZ_PIECE_SCRATCH_MAX || pieces + np > 0x7FFFFFFFull) continue;
        is_split[mi] = 1;
        bytes += 2ull * g.cap; pieces += np;
    }
    uint64_t first = 0, syms = 0;
    for (size_t i = 0; i < n; ++i) {
        pp.first_piece[i] = (uint32_t)first;
        if (!is_split[i]) continue;
        pp.split.push_back((uint32_t)i);
        pp.sym_base[i] = (uint32_t)syms;
        first += ((uint64_t)members[i].body_len + piece_bytes - 1) / piece_bytes;
        syms += members[i].cap;
    }
    pp.first_piece[n] = (uint32_t)first;
    pp.scratch_syms = syms;
    order.erase(std::remove_if(order.begin(), order.end(), [&](uint32_t mi) { return is_split[mi] != 0; }), order.end());
}

}  // namespace mxy
