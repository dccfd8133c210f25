// Whole-line queries (whole_lines.hip): the rules that turn a buffer into a list of queries, as host/device code — the kernels and
// the host tests run the same definitions. A buffer is cut into lines at '\n'; the query of a line is its bytes without one trailing
// '\r'; a query is an address when mxy::parse_ip accepts all of it and a string otherwise; a query that is not valid UTF-8 is not
// looked up. UTF-8 validity is stated per byte, so that it can be decided while the bytes stream: every byte is judged from at most
// three bytes on either side of it, and a line is invalid when one of its bytes is.
#pragma once
#include <cstddef>
#include <cstdint>

#include "netaddr.h"

namespace mxy {
namespace wl {

// A text mxy::parse_ip accepts has at most 45 bytes (six groups of four hex digits, their colons and a dotted quad of 15): a longer
// query is a string without a look at it.
constexpr uint32_t ADDR_TEXT_MAX = 46;
// A query of this many bytes or more is an error of the scan (the length field of a record has 24 bits).
constexpr uint32_t QUERY_LEN_LIMIT = 1u << 24;

enum QueryClass : uint32_t { Q_STRING = 0, Q_IPV4 = 1, Q_IPV6 = 2 };

// Lines of a buffer of `len` bytes that holds `newlines` '\n' bytes and ends in `last` (read only when len > 0): a final piece
// without '\n' is a line, a buffer that ends in '\n' has no empty line behind it.
MXY_ADDR_HD uint32_t line_count(uint32_t len, uint32_t newlines, uint8_t last) { return newlines + ((len && last != '\n') ? 1u : 0u); }

// Line r of the buffer is [line_start, line_end): `ends` holds the positions of the '\n' bytes in ascending order.
MXY_ADDR_HD uint32_t line_start(const uint32_t* ends, uint32_t r) { return r ? ends[r - 1] + 1u : 0u; }
MXY_ADDR_HD uint32_t line_end(const uint32_t* ends, uint32_t newlines, uint32_t len, uint32_t r) { return r < newlines ? ends[r] : len; }

// End of the query of the line [start, end): exactly one trailing '\r' is dropped.
MXY_ADDR_HD uint32_t query_end(const uint8_t* data, uint32_t start, uint32_t end) { return (end > start && data[end - 1] == '\r') ? end - 1u : end; }

// Class of the query q[0, n); `a` is the address when it is one.
MXY_ADDR_HD QueryClass classify(const uint8_t* q, uint32_t n, IpAddr& a) {
    if (n >= ADDR_TEXT_MAX || !parse_ip(reinterpret_cast<const char*>(q), n, a)) return Q_STRING;
    return a.v6 ? Q_IPV6 : Q_IPV4;
}

MXY_ADDR_HD bool utf8_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
// Bytes of the sequence a lead byte begins; 0: the byte begins none (a continuation byte, C0, C1, F5..FF).
MXY_ADDR_HD uint32_t utf8_lead_len(uint32_t b) { return b < 0x80u ? 1u : (b >= 0xC2u && b <= 0xDFu) ? 2u : (b >= 0xE0u && b <= 0xEFu) ? 3u : (b >= 0xF0u && b <= 0xF4u) ? 4u : 0u; }

// Verdict on ONE byte b0 of a buffer (core::str::from_utf8: no overlong forms, no surrogates, nothing above U+10FFFF): true = the
// byte makes its line invalid. m1..m3 are the bytes in front of it (nearest first) of which `back` (0..3) exist, a1..a3 the bytes
// behind it of which `ahead` (0..3) exist; the others are not read.
//  * a lead byte is judged with the sequence it begins: every continuation byte must be there and in the range the lead allows;
//  * a continuation byte must lie inside the sequence of the nearest byte in front of it that is none.
// Every byte of a valid text passes, and a text that is not valid has a byte that fails: the first byte from_utf8 stops at is a lead
// with a bad or missing continuation, a byte that begins nothing, or a continuation byte no sequence reaches.
MXY_ADDR_HD bool utf8_byte_bad(uint32_t m3, uint32_t m2, uint32_t m1, uint32_t b0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t back, uint32_t ahead) {
    if (b0 < 0x80u) return false;
    if (utf8_is_cont(b0)) {
        if (back >= 1 && !utf8_is_cont(m1)) return utf8_lead_len(m1) < 2u;
        if (back >= 2 && !utf8_is_cont(m2)) return utf8_lead_len(m2) < 3u;
        if (back >= 3 && !utf8_is_cont(m3)) return utf8_lead_len(m3) < 4u;
        return true;
    }
    const uint32_t n = utf8_lead_len(b0);
    if (n == 0 || ahead + 1u < n) return true;
    // second byte: the range depends on the lead (E0: no overlong, ED: no surrogate, F0: no overlong, F4: at most U+10FFFF)
    uint32_t lo = 0x80u, hi = 0xBFu;
    if (b0 == 0xE0u) lo = 0xA0u;
    else if (b0 == 0xEDu) hi = 0x9Fu;
    else if (b0 == 0xF0u) lo = 0x90u;
    else if (b0 == 0xF4u) hi = 0x8Fu;
    if (a1 < lo || a1 > hi) return true;
    if (n >= 3 && !utf8_is_cont(a2)) return true;
    if (n >= 4 && !utf8_is_cont(a3)) return true;
    return false;
}

// Byte i of data[0, len) by the rule above (the bytes that do not exist are passed as 0 and not read by the rule).
MXY_ADDR_HD bool utf8_byte_bad_at(const uint8_t* data, uint32_t len, uint32_t i) {
    const uint32_t back = i < 3u ? i : 3u, ahead = len - 1u - i < 3u ? len - 1u - i : 3u;
    return utf8_byte_bad(back >= 3 ? data[i - 3] : 0u, back >= 2 ? data[i - 2] : 0u, back >= 1 ? data[i - 1] : 0u, data[i],
                         ahead >= 1 ? data[i + 1] : 0u, ahead >= 2 ? data[i + 2] : 0u, ahead >= 3 ? data[i + 3] : 0u, back, ahead);
}

}  // namespace wl
}  // namespace mxy
