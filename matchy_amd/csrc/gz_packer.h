// `matchy match --gz-on-gpu`: the packing decisions of the reader. Which .gz input may go to the GPU compressed, which bounds that
// rests on, and when a file opens the next pack. The packer walks the inputs it is given in order, appends the eligible files end to
// end, compressed, and calls back: on_pack with a pack that is complete, not_eligible with an input that keeps the host path — behind
// the pack in hand, so the calls come in input order. What waits (the verdict of the GPU on a pack, the files read again on the host,
// the chain of windows of --gz-windows) is the command line's. Host only (no HIP include) and header-only, like input_packer.h: the
// unit test builds this file with nothing else.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <optional>
#include <string>
#include <vector>

#include "gz_plan.h"
#include "input_packer.h"

namespace mxy {

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// batch_bytes: a batch stays below 2^31 bytes. max_member: the most compressed bytes, and the most ISIZE, of one member (one wave
// inflates it). carry_cap, max_text (--gz-windows): the most bytes a window hands to the next, and the most text of a window's own
// members, so that carry and text fit a batch. The overrides (MATCHY_AMD_GZ_MAX_MEMBER, MATCHY_AMD_GZ_MAX_CARRY) only lower a bound.
struct GzBounds { size_t batch_bytes = 0, max_member = 0, carry_cap = 0; uint64_t max_text = 0; };
inline GzBounds gz_bounds(size_t batch_bytes, std::optional<uint64_t> max_member = {}, std::optional<uint64_t> max_carry = {}) {
    GzBounds b;
    b.batch_bytes = std::min<size_t>(batch_bytes, ((size_t)1 << 31) - ((size_t)1 << 20));
    b.max_member = b.batch_bytes / 4;
    if (max_member) b.max_member = (size_t)std::min<uint64_t>(b.max_member, *max_member);
    b.carry_cap = std::min<size_t>((size_t)1 << 20, b.max_member);
    if (max_carry) b.carry_cap = (size_t)std::min<uint64_t>(b.carry_cap, *max_carry);
    b.max_text = b.batch_bytes - b.carry_cap;   // carry_cap <= max_member <= batch_bytes / 4
    return b;
}

// --gz-pieces: a member is inflated by many waves (inflate_pieces.hip), so one wave's pace no longer bounds it and the member bound is
// what a pack can hold: max_text, and one byte less than a batch for the separator. carry_cap and max_text are those of gz_bounds
// (with the overrides, which lower the member bound here as well).
inline GzBounds gz_bounds_pieces(size_t batch_bytes, std::optional<uint64_t> max_member = {}, std::optional<uint64_t> max_carry = {}) {
    GzBounds b = gz_bounds(batch_bytes, max_member, max_carry);
    b.max_member = (size_t)std::min<uint64_t>(b.max_text, b.batch_bytes - 1);
    if (max_member) b.max_member = (size_t)std::min<uint64_t>(b.max_member, *max_member);
    return b;
}

// One file of a gz pack: its index among the inputs, where it lies in the pack, compressed, and what it vouches for: isize is the sum
// of the ISIZE fields of its `members` members.
struct GzFile { size_t input; uint64_t offset; uint32_t len, isize; uint32_t members = 1; };

// --gz-members: the members of the file p[0, size), whose first header parses. False: a member's compressed length or ISIZE above
// max_member, a piece with no room for its trailer, or more text than one pack holds (the sum of the ISIZEs plus the separator).
inline bool gz_members_fit(const uint8_t* p, size_t size, const GzBounds& b, std::vector<uint64_t>& cuts, uint32_t& n_members, uint32_t& isize) {
    gz_split_members(p, size, cuts);
    uint64_t sum = 0;
    for (size_t k = 0; k < cuts.size(); ++k) {
        const uint64_t at = cuts[k], len = (k + 1 < cuts.size() ? cuts[k + 1] : (uint64_t)size) - at;
        uint64_t body = 0;
        if (len > b.max_member || gz_parse_header(p + at, len, body) != GZ_PLAN_OK || len - body < 8) return false;
        const uint32_t is = le32(p + at + len - 4);
        if (is > b.max_member) return false;
        sum += is;
        if (sum + 1 > b.batch_bytes) return false;
    }
    n_members = (uint32_t)cuts.size(); isize = (uint32_t)sum;
    return true;
}

// Eligibility, in front of the read: the name ends in .gz (any case) and is a regular file of at least 18 bytes (the smallest member)
// and at most max_member — with --gz-members at most batch_bytes: a file may be as large as a pack, its members are what must be small.
inline bool gz_eligible_file(const std::string& path, const GzBounds& b, bool members, size_t& size) {
    struct stat sb;
    if (!pack_ends_with_gz(path) || stat(path.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode) || sb.st_size < 18) return false;
    size = (size_t)sb.st_size;
    return size <= (members ? b.batch_bytes : b.max_member);
}
// Eligibility, behind the read, of the whole file p[0, size): the first header parses and leaves room for the trailer; with
// --gz-members its members fit; a file of one member is held to max_member, compressed and inflated, with the flag and without.
inline bool gz_eligible_bytes(const uint8_t* p, size_t size, const GzBounds& b, bool members, std::vector<uint64_t>& cuts, uint32_t& n_members, uint32_t& isize) {
    uint64_t body = 0;
    if (gz_parse_header(p, size, body) != GZ_PLAN_OK || size - body < 8) return false;
    n_members = 1; isize = le32(p + size - 4);
    if (members && !gz_members_fit(p, size, b, cuts, n_members, isize)) return false;
    return n_members > 1 || (size <= b.max_member && isize <= b.max_member);
}

// The pack in hand. A pack holds up to batch_bytes of inflated text, one separator behind every file counted in, and goes out when the
// next file would pass that — with --gz-members also when its compressed bytes would pass batch_bytes, where a file of many empty
// members may be as large as a pack and vouch for no text.
struct GzPacker {
    GzBounds bounds;
    bool members = false;   // --gz-members: files of many members are eligible
    std::function<void(const std::vector<uint8_t>& packed, const std::vector<GzFile>& files)> on_pack;
    std::function<void(size_t input)> not_eligible;
    std::function<long long(const std::string&, uint8_t*, size_t)> read_file = pack_read_file;   // the bytes read, as pack_read_file

    std::vector<uint8_t> buf;     // the files of the pack in hand, compressed, end to end
    std::vector<GzFile> files;
    uint64_t text = 0;            // inflated bytes of the pack in hand, separators included
    std::vector<uint64_t> cuts;

    void take(size_t i, const std::string& path) {
        size_t size = 0;
        if (!gz_eligible_file(path, bounds, members, size)) return leave(i);
        const size_t at = buf.size();
        buf.resize(at + size);
        uint32_t isize = 0, n_members = 1;
        // a file that shrank behind the stat is not whole
        if (read_file(path, buf.data() + at, size) != (long long)size || !gz_eligible_bytes(buf.data() + at, size, bounds, members, cuts, n_members, isize)) {
            buf.resize(at);
            return leave(i);
        }
        if (!files.empty() && (text + isize + 1 > bounds.batch_bytes || (members && at + size > bounds.batch_bytes))) {   // opens the next pack
            const std::vector<uint8_t> file(buf.begin() + (long)at, buf.end());
            buf.resize(at);
            flush();
            buf = file;
        }
        files.push_back(GzFile{i, buf.size() - size, (uint32_t)size, isize, n_members});
        text += (uint64_t)isize + 1;
    }
    void flush() {
        if (files.empty()) return;
        on_pack(buf, files);
        buf.clear(); files.clear(); text = 0;
    }
    void leave(size_t i) { flush(); not_eligible(i); }
};

}  // namespace mxy
