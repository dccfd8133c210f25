// NDJSON records of a scan result: everything that decides a byte of the output, as host/device code. record_emit() below is the
// grammar of a record; its users are the host renderer (ndjson_host.cpp), the kernels of render.hip, the sequential model of their
// test and the CPU test (tests/cpp/test_render_core.cpp). None of them spells a key, a literal or the "cidr" rule itself.
//
// A record is a sequence of parts, emitted by record_emit() into a SINK: literals, decimal numbers, verbatim bytes (payload JSON and
// the escaped source, both made by the host) and the two escaped fields, "matched_text" (json_escape of the raw bytes) and
// "input_line" (json_escape of utf8_lossy of the line). A sink that counts gives the length of a record, a sink that stores writes
// it; render.hip adds sinks in which the lanes of a wave share the work.
//
// Both escaped fields are stated PER BYTE: byte i of a field of n bytes contributes a fixed text that depends on the bytes
// i-3 .. i+3 inside the field and on nothing else (bytes outside the field do not exist). A field can therefore be cut at any
// position into pieces that are measured and written independently; the pieces concatenate to the text of the whole.
#pragma once
#include <cstddef>
#include <cstdint>

#include "netaddr.h"

#if defined(__HIPCC__)
#define MXY_RC_HD __host__ __device__ inline
#else
#define MXY_RC_HD inline
#endif

namespace mxy {
namespace render {

constexpr uint32_t FLAG_LINE_NUMBERS = 1u;   // MATCHY_RENDER_LINE_NUMBERS
constexpr uint32_t FLAG_INPUT_LINE = 2u;     // MATCHY_RENDER_INPUT_LINE (implies line numbers)
constexpr uint32_t BYTE_TEXT_MAX = 6;        // the longest text of one byte: \u00xx

// ------------------------------------------------------------------------------------------------ numbers
MXY_RC_HD uint32_t dec_len(uint64_t v) {
    uint32_t n = 1;
    for (; v >= 10; v /= 10) ++n;   // at most 20 digits
    return n;
}
MXY_RC_HD uint32_t dec_put(uint64_t v, uint8_t* o) {
    const uint32_t n = dec_len(v);
    for (uint32_t k = n; k-- > 0; v /= 10) o[k] = (uint8_t)('0' + v % 10);
    return n;
}

// ------------------------------------------------------------------------------------------------ json_escape, one byte
MXY_RC_HD uint32_t esc_len(uint8_t c) {
    if (c == '"' || c == 0x5C) return 2;
    if (c >= 0x20) return 1;   // bytes >= 0x7F pass through
    return (c == '\b' || c == '\f' || c == '\n' || c == '\r' || c == '\t') ? 2 : 6;
}
MXY_RC_HD uint32_t esc_put(uint8_t c, uint8_t* o) {
    const uint32_t n = esc_len(c);
    if (n == 1) { o[0] = c; return 1; }
    o[0] = 0x5C;
    if (n == 2) {
        o[1] = c == '\b' ? 'b' : c == '\f' ? 'f' : c == '\n' ? 'n' : c == '\r' ? 'r' : c == '\t' ? 't' : c;
        return 2;
    }
    o[1] = 'u'; o[2] = '0'; o[3] = '0';
    o[4] = (uint8_t)('0' + (c >> 4));   // c < 0x20: the high digit is 0 or 1
    o[5] = (uint8_t)((c & 15) < 10 ? '0' + (c & 15) : 'a' + ((c & 15) - 10));
    return 6;
}

// ------------------------------------------------------------------------------------------------ utf8_lossy + json_escape, one byte
// The rule of utf8_lossy.h (one U+FFFD per maximal ill-formed subsequence) as a function of position. Who begins a sequence is decided
// locally: a byte outside 0x80..0xBF always begins one (it is never consumed as a continuation), and a byte inside that range belongs
// to the lead byte that is the nearest byte outside the range in front of it iff that lead lies at most three bytes back, asks for
// that many continuations and accepts every byte from itself up to here. A complete sequence passes through, one byte each; an
// incomplete one gives U+FFFD at its lead and nothing at the continuations it consumed; any other byte >= 0x80 is U+FFFD by itself.
struct Utf8Lead { uint32_t need; uint8_t lo, hi; };   // continuation bytes asked for (0: not a lead), range of the first of them
MXY_RC_HD Utf8Lead utf8_lead(uint8_t c) {
    Utf8Lead l{0, 0x80, 0xBF};
    if (c >= 0xC2 && c <= 0xDF) l.need = 1;
    else if (c >= 0xE0 && c <= 0xEF) { l.need = 2; if (c == 0xE0) l.lo = 0xA0; if (c == 0xED) l.hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { l.need = 3; if (c == 0xF0) l.lo = 0x90; if (c == 0xF4) l.hi = 0x8F; }
    return l;
}
// bytes of the sequence that begins with the lead at `at` which are well-formed (1 .. need + 1; need + 1: complete)
MXY_RC_HD uint32_t utf8_accepted(const uint8_t* f, uint32_t n, uint32_t at, Utf8Lead l) {
    uint32_t k = 1;
    for (; k <= l.need; ++k) {   // at most three bytes ahead
        if (at + k >= n) break;
        const uint8_t b = f[at + k];
        if (k == 1 ? (b < l.lo || b > l.hi) : ((b & 0xC0) != 0x80)) break;
    }
    return k;
}
enum : uint32_t { U8_ASCII = 0, U8_COPY = 1, U8_REPLACE = 2, U8_NOTHING = 3 };
MXY_RC_HD uint32_t utf8_role(const uint8_t* f, uint32_t n, uint32_t i) {
    const uint8_t c = f[i];
    if (c < 0x80) return U8_ASCII;
    if ((c & 0xC0) != 0x80) {   // begins a sequence
        const Utf8Lead l = utf8_lead(c);
        if (!l.need) return U8_REPLACE;
        return utf8_accepted(f, n, i, l) == l.need + 1 ? U8_COPY : U8_REPLACE;
    }
    for (uint32_t d = 1; d <= 3 && d <= i; ++d) {   // at most three bytes back
        const uint8_t p = f[i - d];
        if ((p & 0xC0) == 0x80) continue;
        const Utf8Lead l = utf8_lead(p);
        if (l.need < d) break;
        const uint32_t k = utf8_accepted(f, n, i - d, l);
        if (k <= d) break;   // the sequence ended in front of this byte
        return k == l.need + 1 ? U8_COPY : U8_NOTHING;
    }
    return U8_REPLACE;   // a continuation byte without a lead
}
MXY_RC_HD uint32_t line_byte_len(const uint8_t* f, uint32_t n, uint32_t i) {
    const uint32_t role = utf8_role(f, n, i);
    return role == U8_ASCII ? esc_len(f[i]) : role == U8_COPY ? 1u : role == U8_REPLACE ? 3u : 0u;
}
MXY_RC_HD uint32_t line_byte_put(const uint8_t* f, uint32_t n, uint32_t i, uint8_t* o) {
    const uint32_t role = utf8_role(f, n, i);
    if (role == U8_ASCII) return esc_put(f[i], o);
    if (role == U8_COPY) { o[0] = f[i]; return 1; }
    if (role == U8_NOTHING) return 0;
    o[0] = 0xEF; o[1] = 0xBF; o[2] = 0xBD;
    return 3;
}

// bytes [a, b) of a field of n bytes, sequentially: the length of their text, and the text itself at o
MXY_RC_HD uint64_t text_piece_len(const uint8_t* f, uint32_t a, uint32_t b) {
    uint64_t t = 0;
    for (uint32_t i = a; i < b; ++i) t += esc_len(f[i]);
    return t;
}
MXY_RC_HD uint64_t line_piece_len(const uint8_t* f, uint32_t n, uint32_t a, uint32_t b) {
    uint64_t t = 0;
    for (uint32_t i = a; i < b; ++i) t += line_byte_len(f, n, i);
    return t;
}

// ------------------------------------------------------------------------------------------------ sinks
// what a sink offers: lit (program text), bytes (verbatim), text / text_inline (json_escape of raw bytes, without the quotes),
// line (json_escape of utf8_lossy, without the quotes), dec. text and line are the two fields render.hip cuts into pieces;
// text_inline is the same rule for the few bytes of an address that did not parse.
struct LenSink {
    uint64_t n = 0;
    MXY_RC_HD void lit(const char*, uint32_t len) { n += len; }
    MXY_RC_HD void bytes(const uint8_t*, uint32_t len) { n += len; }
    MXY_RC_HD void text(const uint8_t* f, uint32_t len) { n += text_piece_len(f, 0, len); }
    MXY_RC_HD void text_inline(const uint8_t* f, uint32_t len) { text(f, len); }
    MXY_RC_HD void line(const uint8_t* f, uint32_t len) { n += line_piece_len(f, len, 0, len); }
    MXY_RC_HD void dec(uint64_t v) { n += dec_len(v); }
};
// stores the bytes whose position in the block lies in front of `end` and no others; pos counts past it
struct PutSink {
    uint8_t* o;
    uint64_t pos, end;
    MXY_RC_HD void put(const uint8_t* p, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) if (pos + k < end) o[pos + k] = p[k];
        pos += len;
    }
    MXY_RC_HD void lit(const char* p, uint32_t len) { put(reinterpret_cast<const uint8_t*>(p), len); }
    MXY_RC_HD void bytes(const uint8_t* p, uint32_t len) { put(p, len); }
    MXY_RC_HD void text(const uint8_t* f, uint32_t len) {
        uint8_t t[BYTE_TEXT_MAX];
        for (uint32_t i = 0; i < len; ++i) put(t, esc_put(f[i], t));
    }
    MXY_RC_HD void text_inline(const uint8_t* f, uint32_t len) { text(f, len); }
    MXY_RC_HD void line(const uint8_t* f, uint32_t len) {
        uint8_t t[BYTE_TEXT_MAX];
        for (uint32_t i = 0; i < len; ++i) put(t, line_byte_put(f, len, i, t));
    }
    MXY_RC_HD void dec(uint64_t v) { uint8_t t[20]; put(t, dec_put(v, t)); }
};

// ------------------------------------------------------------------------------------------------ one record
struct RecordIn {
    const uint8_t* hit;       // the matched text
    uint32_t hit_len;
    uint32_t value;           // IP: data offset of the payload; pattern: index of the first id
    uint32_t n_ids;           // pattern results
    uint8_t kind;             // 2 = IP result, 3 = pattern result
    uint8_t prefix_len;
    uint32_t flags;           // FLAG_*
    const uint8_t* line;      // FLAG_INPUT_LINE: the line of the hit, without its terminator
    uint32_t line_len;
    uint64_t line_number;     // FLAG_LINE_NUMBERS: as printed (base + line + 1)
    const uint8_t* source;    // the escaped source with its quotes
    uint32_t source_len;
};

#define MXY_RC_LIT(s, str) (s).lit(str, (uint32_t)sizeof(str) - 1u)

// "cidr": format_cidr(parse_ip(T), P), or json_escape(T + "/" + P) where T does not parse. The parser's loops are bounded by
// its digit limits, not by the length of T.
template <class Sink>
MXY_RC_HD void cidr_emit(const uint8_t* hit, uint32_t hit_len, uint32_t prefix, Sink& s) {
    IpAddr ip;
    MXY_RC_LIT(s, "\"");
    if (parse_ip(reinterpret_cast<const char*>(hit), hit_len, ip)) {
        char c[IP_CIDR_TEXT_MAX];
        s.lit(c, format_cidr_to(ip, prefix, c));   // digits, ':', '.', '/': nothing to escape
    } else {
        s.text_inline(hit, hit_len);
        MXY_RC_LIT(s, "/");
        s.dec(prefix);
    }
    MXY_RC_LIT(s, "\"");
}

// Payloads: one(sink, data offset) emits the payload JSON of an IP result; array(sink, first, n_ids) emits `"data":[D0,D1,...],`
// for the ids with a data offset >= 0, or nothing where there is none. How they find the texts is the caller's business.
template <class Sink, class Payloads>
MXY_RC_HD void record_emit(const RecordIn& r, Payloads& pay, Sink& s) {
    if (r.kind == 2) {
        MXY_RC_LIT(s, "{\"cidr\":");
        cidr_emit(r.hit, r.hit_len, r.prefix_len, s);
        MXY_RC_LIT(s, ",\"data\":");
        pay.one(s, r.value);
        MXY_RC_LIT(s, ",");
    } else {
        MXY_RC_LIT(s, "{");
        pay.array(s, r.value, r.n_ids);
    }
    if (r.flags & FLAG_INPUT_LINE) {
        MXY_RC_LIT(s, "\"input_line\":\"");
        s.line(r.line, r.line_len);
        MXY_RC_LIT(s, "\",");
    }
    if (r.flags & (FLAG_LINE_NUMBERS | FLAG_INPUT_LINE)) {
        MXY_RC_LIT(s, "\"line_number\":");
        s.dec(r.line_number);
        MXY_RC_LIT(s, ",");
    }
    if (r.kind == 2) MXY_RC_LIT(s, "\"match_type\":\"ip\",\"matched_text\":\"");
    else MXY_RC_LIT(s, "\"match_type\":\"pattern\",\"matched_text\":\"");
    s.text(r.hit, r.hit_len);
    if (r.kind == 2) { MXY_RC_LIT(s, "\",\"prefix_len\":"); s.dec(r.prefix_len); }
    else { MXY_RC_LIT(s, "\",\"pattern_count\":"); s.dec(r.n_ids); }
    MXY_RC_LIT(s, ",\"source\":");
    s.bytes(r.source, r.source_len);
    MXY_RC_LIT(s, ",\"timestamp\":\"0.000\"}\n");
}

}  // namespace render
}  // namespace mxy
