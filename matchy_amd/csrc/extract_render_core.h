// Extracted candidates as text (`matchy extract`): everything that decides the order of the candidates of a batch and a byte of their
// output, as host/device code. Its users are the kernels of extract_render.hip, the sequential model of their test and the CPU test
// (tests/cpp/test_extract_render_core.cpp). The rules are those of extract_batch (cli_main.cpp), which prints the same bytes on the host.
//
// Order: (line, rank, start) — the number of '\n' bytes in front of the candidate, the line order of the item types (line_rank of
// cli_main.cpp; NOT the chunk-path order of distinct_type_rank), the start offset. The triple is one 64-bit key, so a sort by key is a
// sort by triple. No two candidates of a batch share (rank, start).
//
// Text of one candidate, <name> the item type's name in lower case, <bytes> the raw bytes data[start, start + len):
//   json   {"type":"<name>","value":"<bytes>"}\n   with \ -> \\ and " -> \" and no other escape
//   csv    <name>,"<bytes>"\n                      with " doubled
//   text   <bytes>\n
#pragma once
#include <cstddef>
#include <cstdint>

#include "hashes.h"
#include "scan_types.h"

namespace mxy {
namespace xrender {

constexpr uint32_t FORMAT_JSON = 0, FORMAT_CSV = 1, FORMAT_TEXT = 2, FORMAT_COUNT = 3;   // MATCHY_AMD_EXTRACT_FORMAT_*

// ------------------------------------------------------------------------------------------------ order
constexpr uint32_t LINE_BITS = 31, RANK_BITS = 3, START_BITS = 30;
static_assert(LINE_BITS + RANK_BITS + START_BITS == 64, "the triple fills the key");
constexpr uint32_t MAX_LEN = 1u << START_BITS;   // bytes of one launch: starts (and so lines) stay below it
constexpr uint32_t RANKS = 1u << RANK_BITS;

MXY_HD uint32_t rank(uint32_t item_type) {
    switch (item_type) {
        case IT_DOMAIN: return 0; case IT_IPV4: return 1; case IT_EMAIL: return 2; case IT_IPV6: return 3;
        case IT_BITCOIN: return 5; case IT_ETHEREUM: return 6; case IT_MONERO: return 7;
    }
    return 4;   // the hash types
}
MXY_HD unsigned long long key_pack(uint32_t line, uint32_t rank, uint32_t start) {
    return ((unsigned long long)line << (RANK_BITS + START_BITS)) | ((unsigned long long)rank << START_BITS) | (unsigned long long)start;
}
MXY_HD uint32_t key_line(unsigned long long k) { return (uint32_t)(k >> (RANK_BITS + START_BITS)); }
MXY_HD uint32_t key_rank(unsigned long long k) { return (uint32_t)(k >> START_BITS) & (RANKS - 1u); }
MXY_HD uint32_t key_start(unsigned long long k) { return (uint32_t)k & (MAX_LEN - 1u); }

// ------------------------------------------------------------------------------------------------ text
constexpr uint32_t TYPE_NAME_MAX = 8, HEAD_MAX = 9 + TYPE_NAME_MAX + 11, TAIL_MAX = 3;

// item_type_name in lower case; an unknown type prints as "unknown"
MXY_HD uint32_t name_put(uint32_t item_type, uint8_t* o) {
    const char* s;
    switch (item_type) {
        case IT_DOMAIN: s = "domain"; break;     case IT_EMAIL: s = "email"; break;       case IT_IPV4: s = "ipv4"; break;
        case IT_IPV6: s = "ipv6"; break;         case IT_MD5: s = "md5"; break;           case IT_SHA1: s = "sha1"; break;
        case IT_SHA256: s = "sha256"; break;     case IT_SHA384: s = "sha384"; break;     case IT_SHA512: s = "sha512"; break;
        case IT_BITCOIN: s = "bitcoin"; break;   case IT_ETHEREUM: s = "ethereum"; break; case IT_MONERO: s = "monero"; break;
        default: s = "unknown";
    }
    uint32_t n = 0;
    for (; s[n]; ++n) o[n] = (uint8_t)s[n];   // at most TYPE_NAME_MAX
    return n;
}
MXY_HD uint32_t name_len(uint32_t item_type) {
    uint8_t t[TYPE_NAME_MAX];
    return name_put(item_type, t);
}
MXY_HD uint32_t lit_put(const char* s, uint8_t* o) {
    uint32_t n = 0;
    for (; s[n]; ++n) o[n] = (uint8_t)s[n];
    return n;
}

// what stands in front of <bytes> and behind it
MXY_HD uint32_t head_put(uint32_t format, uint32_t item_type, uint8_t* o) {
    uint32_t n = 0;
    if (format == FORMAT_JSON) {
        n += lit_put("{\"type\":\"", o);
        n += name_put(item_type, o + n);
        n += lit_put("\",\"value\":\"", o + n);
    } else if (format == FORMAT_CSV) {
        n += name_put(item_type, o);
        n += lit_put(",\"", o + n);
    }
    return n;
}
MXY_HD uint32_t head_len(uint32_t format, uint32_t item_type) {
    return format == FORMAT_JSON ? 9u + name_len(item_type) + 11u : format == FORMAT_CSV ? name_len(item_type) + 2u : 0u;
}
MXY_HD uint32_t tail_put(uint32_t format, uint8_t* o) {
    return format == FORMAT_JSON ? lit_put("\"}\n", o) : format == FORMAT_CSV ? lit_put("\"\n", o) : lit_put("\n", o);
}
MXY_HD uint32_t tail_len(uint32_t format) { return format == FORMAT_JSON ? 3u : format == FORMAT_CSV ? 2u : 1u; }

// one byte of <bytes>: 1 where it takes a second byte in the output
MXY_HD uint32_t is_escape(uint32_t format, uint8_t c) {
    return (format == FORMAT_JSON && (c == '"' || c == 0x5C)) || (format == FORMAT_CSV && c == '"') ? 1u : 0u;
}
MXY_HD uint32_t byte_put(uint32_t format, uint8_t c, uint8_t* o) {
    if (!is_escape(format, c)) { o[0] = c; return 1; }
    o[0] = format == FORMAT_JSON ? (uint8_t)0x5C : (uint8_t)'"';
    o[1] = c;
    return 2;
}
MXY_HD uint64_t count_escapes(uint32_t format, const uint8_t* f, uint32_t len) {
    uint64_t n = 0;
    for (uint32_t i = 0; i < len; ++i) n += is_escape(format, f[i]);
    return n;
}

// length of a record from (type, len, escapes)
MXY_HD uint64_t record_len(uint32_t format, uint32_t item_type, uint32_t len, uint64_t escapes) {
    return (uint64_t)head_len(format, item_type) + len + escapes + tail_len(format);
}

// The record of the candidate f[0, len), written at block position `pos`: stores the bytes whose position lies in front of `end` and no
// others. Returns the length of the record.
MXY_HD uint64_t record_put(uint32_t format, uint32_t item_type, const uint8_t* f, uint32_t len, uint8_t* block, uint64_t pos, uint64_t end) {
    const uint64_t at = pos;
    uint8_t t[HEAD_MAX];
    uint32_t n = head_put(format, item_type, t);
    for (uint32_t k = 0; k < n; ++k) if (pos + k < end) block[pos + k] = t[k];
    pos += n;
    for (uint32_t i = 0; i < len; ++i) {
        n = byte_put(format, f[i], t);
        for (uint32_t k = 0; k < n; ++k) if (pos + k < end) block[pos + k] = t[k];
        pos += n;
    }
    n = tail_put(format, t);
    for (uint32_t k = 0; k < n; ++k) if (pos + k < end) block[pos + k] = t[k];
    pos += n;
    return pos - at;
}

}  // namespace xrender
}  // namespace mxy
