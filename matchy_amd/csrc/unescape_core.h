// Percent- and JSON-escaped text, decoded: the one definition of the two grammars, for the kernels (unescape.hip) and for a CPU driver
// (tests). Host and device; the host needs no HIP include.
//
// Every input position emits 0 to 4 bytes. The bytes of a valid escape are consumed: its first byte owns the output, the others emit
// nothing. Every other byte is literal and emits itself.
//   PERCENT  '%' and two hex digits (either case), all inside the input: the byte with that value. Nothing else: '+' stays '+', "%25"
//            becomes '%' once, '%' with fewer than two hex digits behind it is literal.
//   JSON     esc[i] = data[i-1] == '\\' && !esc[i-1], esc[0] = 0; a backslash with esc == 0 is an introducer.
//            introducer + one of " \ / b f n r t      two-byte escape for the byte it names
//            introducer + 'u' + four hex digits       six-byte escape for a UTF-16 code unit, written as UTF-8. A high surrogate escape
//                                                     with a low one directly behind it: the four bytes of the pair, the low one emits
//                                                     nothing. Any other surrogate escape: EF BF BD, one per escape (utf16_core.h's rule)
//            introducer + anything else               no escape: both bytes emit themselves (\u with fewer than four hex digits, '\\' in
//                                                     front of a real LF, '\\' as the last byte). The byte behind it still counts as
//                                                     escaped for esc[].
// Line ends, both modes: a real 0x0A emits itself; an escape whose value is LF (%0A, \n, \u000a) is written as one space. The decoded text
// has exactly the LF bytes of the input, and since no escape spans a real LF, decode(A + B) == decode(A) + decode(B) for a cut behind an LF.
// JSON | PERCENT is percent(json(x)): two runs of the pass, no fused grammar. The output is never longer than the input.
//
// A position is decided from a Window: the 16 bytes of a lane, LOOK_BEHIND bytes in front, LOOK_AHEAD behind (a surrogate pair is twelve
// bytes: the high escape looks at 11 bytes behind its backslash, the low one at the 6 in front), and the esc bits of the first 22.
// item_len and item_bytes are the only place where a position's output is decided (both are decode()): a count pass and a write pass
// that are built from them cannot disagree.
//
// esc at a tile's first byte depends on the parity of the backslash run in front of it, which may span many tiles. A tile's 7-bit STATE
// is esc of its first byte (bit 0) and of the six bytes in front of it (bits 1..6, oldest first). What a full tile hands to the next one
// is one of two states, by its own state's bit 0: its CODE (state for bit 0 = 0 in bits 0..6, for bit 0 = 1 in bits 8..14). On bit 0 a
// code is one of four functions — constant 0, constant 1, identity (a tile of backslashes) or negation — which compose associatively
// (fn_of, fn_compose), so the states of all tiles come from a scan over the codes.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MXY_UNESC_HD __host__ __device__ __forceinline__
#define MXY_UNESC_UNROLL _Pragma("unroll")   // the windows stay in registers: every index is a constant once the loops are unrolled
#else
#define MXY_UNESC_HD inline
#define MXY_UNESC_UNROLL
#endif

namespace mxy {
namespace unescape {

constexpr uint32_t MODE_PERCENT = 1, MODE_JSON = 2;
constexpr uint32_t BYTE_NONE = 0x100u;   // no byte: in front of the input or behind it
// Work partition of the passes: a tile is TILE_BYTES input bytes, a lane has LANE_BYTES of them. A position emits more than one byte
// only where at least five consumed ones follow, so a tile gives most when a surrogate-pair escape begins on its last byte: 1023 + 4.
constexpr uint32_t TILE_BYTES = 1024, LANE_BYTES = 16, TILE_LANES = TILE_BYTES / LANE_BYTES, TILE_OUT_MAX = TILE_BYTES + 3;
constexpr uint32_t LOOK_BEHIND = 6, LOOK_AHEAD = 11, OWN = LOOK_BEHIND, WINDOW_BYTES = LOOK_BEHIND + LANE_BYTES + LOOK_AHEAD;
static_assert(TILE_OUT_MAX == TILE_BYTES - 1 + 4, "the last position of a tile may own the four bytes of a surrogate pair");

// b[OWN + k]: byte k of the lane; esc bit j: b[j] is escaped (j < OWN + LANE_BYTES; JSON only)
struct Window { uint32_t b[WINDOW_BYTES]; uint32_t esc; };

constexpr uint32_t F_ESCAPE = 1, F_REPLACED = 2, F_LF = 4;
struct Item { uint32_t len, bytes, flags; };   // bytes: first byte in bits 0..7; flags: what the position adds to the counters

MXY_UNESC_HD int hex_value(uint32_t c) {
    if (c - '0' < 10u) return (int)(c - '0');
    const uint32_t l = (c | 0x20u) - 'a';
    return l < 6u ? (int)(l + 10u) : -1;   // BYTE_NONE | 0x20 is no letter
}
MXY_UNESC_HD int hex2(const Window& w, uint32_t j) {
    const int a = hex_value(w.b[j]), b = hex_value(w.b[j + 1]);
    return (a | b) < 0 ? -1 : (a << 4) | b;
}
MXY_UNESC_HD int hex4(const Window& w, uint32_t j) {
    const int a = hex2(w, j), b = hex2(w, j + 2);
    return (a | b) < 0 ? -1 : (a << 8) | b;
}
MXY_UNESC_HD int json_simple(uint32_t c) {
    switch (c) {
        case '"': return 0x22; case '\\': return 0x5C; case '/': return 0x2F; case 'b': return 0x08;
        case 'f': return 0x0C; case 'n': return 0x0A; case 'r': return 0x0D; case 't': return 0x09;
        default: return -1;
    }
}
// the code unit of "\uXXXX" at b[j .. j + 5], -1 where those bytes are no such text (esc of b[j] is the caller's matter)
MXY_UNESC_HD int json_unit(const Window& w, uint32_t j) { return w.b[j] == '\\' && w.b[j + 1] == 'u' ? hex4(w, j + 2) : -1; }
MXY_UNESC_HD bool is_high(int u) { return (u & ~0x3FF) == 0xD800; }
MXY_UNESC_HD bool is_low(int u) { return (u & ~0x3FF) == 0xDC00; }

MXY_UNESC_HD Item literal(uint32_t x) { return Item{1, x, 0}; }
MXY_UNESC_HD Item consumed() { return Item{0, 0, 0}; }
// a decoded code unit that is no surrogate, as UTF-8; LF as a space
MXY_UNESC_HD Item decoded(uint32_t v) {
    if (v == 0x0Au) return Item{1, 0x20u, F_ESCAPE | F_LF};
    if (v < 0x80u) return Item{1, v, F_ESCAPE};
    if (v < 0x800u) return Item{2, (0xC0u | (v >> 6)) | ((0x80u | (v & 0x3Fu)) << 8), F_ESCAPE};
    return Item{3, (0xE0u | (v >> 12)) | ((0x80u | ((v >> 6) & 0x3Fu)) << 8) | ((0x80u | (v & 0x3Fu)) << 16), F_ESCAPE};
}

// a decoded byte as it is (PERCENT: bytes, not code points); LF as a space
MXY_UNESC_HD Item decoded_byte(uint32_t v) { return v == 0x0Au ? Item{1, 0x20u, F_ESCAPE | F_LF} : Item{1, v, F_ESCAPE}; }

MXY_UNESC_HD Item decode_percent(const Window& w, uint32_t p) {
    const uint32_t x = w.b[p];
    if (x == BYTE_NONE) return consumed();
    if (x == '%') {
        const int v = hex2(w, p + 1);
        return v < 0 ? literal(x) : decoded_byte((uint32_t)v);
    }
    if (hex_value(x) >= 0) {   // a digit of an escape: '%' is no digit, so a '%' with two digits behind it is always an escape
        if (w.b[p - 1] == '%' && hex_value(w.b[p + 1]) >= 0) return consumed();
        if (w.b[p - 2] == '%' && hex_value(w.b[p - 1]) >= 0) return consumed();
    }
    return literal(x);
}

MXY_UNESC_HD Item decode_json(const Window& w, uint32_t p) {
    const uint32_t x = w.b[p];
    if (x == BYTE_NONE) return consumed();
    if ((w.esc >> p) & 1u) {   // the byte behind an introducer
        if (json_simple(x) >= 0 || (x == 'u' && hex4(w, p + 1) >= 0)) return consumed();
        return literal(x);
    }
    if (x == '\\') {           // an introducer
        const uint32_t c = w.b[p + 1];
        const int v = json_simple(c);
        if (v >= 0) return decoded((uint32_t)v);
        const int u = c == 'u' ? hex4(w, p + 2) : -1;
        if (u < 0) return literal(x);
        if (is_high(u)) {
            const int lo = json_unit(w, p + 6);   // b[p + 5] is a digit, so a backslash at p + 6 is an introducer
            if (!is_low(lo)) return Item{3, 0x00BDBFEFu, F_ESCAPE | F_REPLACED};
            const uint32_t cp = 0x10000u + (((uint32_t)u & 0x3FFu) << 10) + ((uint32_t)lo & 0x3FFu);
            return Item{4, (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 0x3Fu)) << 8) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 16) | ((0x80u | (cp & 0x3Fu)) << 24), F_ESCAPE};
        }
        if (is_low(u)) {
            if (!((w.esc >> (p - 6)) & 1u) && is_high(json_unit(w, p - 6))) return Item{0, 0, F_ESCAPE};   // the high one wrote the pair
            return Item{3, 0x00BDBFEFu, F_ESCAPE | F_REPLACED};
        }
        return decoded((uint32_t)u);
    }
    if (hex_value(x) >= 0) {   // a digit of a unit escape whose introducer lies 2 to 5 bytes in front
        MXY_UNESC_UNROLL
        for (uint32_t k = 2; k <= 5; ++k)
            if (!((w.esc >> (p - k)) & 1u) && json_unit(w, p - k) >= 0) return consumed();
    }
    return literal(x);
}

// What position b[p] (OWN <= p < OWN + LANE_BYTES) of the window emits. mode: MODE_PERCENT or MODE_JSON.
MXY_UNESC_HD Item decode(const Window& w, uint32_t p, uint32_t mode) { return mode == MODE_JSON ? decode_json(w, p) : decode_percent(w, p); }
MXY_UNESC_HD uint32_t item_len(const Window& w, uint32_t p, uint32_t mode) { return decode(w, p, mode).len; }
MXY_UNESC_HD uint32_t item_bytes(const Window& w, uint32_t p, uint32_t mode) { return decode(w, p, mode).bytes; }
MXY_UNESC_HD uint32_t item_flags(const Window& w, uint32_t p, uint32_t mode) { return decode(w, p, mode).flags; }

// Every position of a lane is literal when no byte that opens an escape lies in its own bytes or close enough in front of them to
// consume one of them: '%' up to 2 bytes in front, '\\' up to 5 (a low surrogate escape has its own backslash).
MXY_UNESC_HD bool lane_is_literal(const Window& w, uint32_t mode) {
    const uint32_t c = mode == MODE_JSON ? '\\' : '%';
    bool any = false;
    MXY_UNESC_UNROLL
    for (uint32_t j =OWN - (mode == MODE_JSON ? 5u : 2u); j < OWN + LANE_BYTES; ++j) any |= w.b[j] == c;
    return !any;
}

// esc of the lane's own bytes (bit k: b[OWN + k]) from esc of its first byte; *out: esc of the byte behind the lane
MXY_UNESC_HD uint32_t lane_esc(const Window& w, uint32_t e, uint32_t* out = nullptr) {
    uint32_t m = 0;
    MXY_UNESC_UNROLL
    for (uint32_t k = 0; k < LANE_BYTES; ++k) {
        m |= e << k;
        e = (w.b[OWN + k] == '\\') & (e ^ 1u);
    }
    if (out) *out = e;
    return m;
}

// ---- the state of a tile --------------------------------------------------------------------------------------------------------------
constexpr uint32_t STATE_MASK = 0x7Fu;
MXY_UNESC_HD uint32_t code_apply(uint32_t code, uint32_t state) { return (code >> (8u * (state & 1u))) & STATE_MASK; }
// a code as a function on bit 0: bit s of the result = f(s). 0: constant 0, 3: constant 1, 2: identity, 1: negation
MXY_UNESC_HD uint32_t fn_of(uint32_t code) { return (code & 1u) | ((code >> 7) & 2u); }
constexpr uint32_t FN_IDENTITY = 2u;
MXY_UNESC_HD uint32_t fn_compose(uint32_t first, uint32_t then) { return ((then >> (first & 1u)) & 1u) | (((then >> ((first >> 1) & 1u)) & 1u) << 1); }
// The code of a tile from its last 16 bytes (tail[k], no BYTE_NONE among them) once esc of tail[from] is known for both states (e0: bit s
// = esc for state bit 0 = s); from <= 10, so the six esc bits of the next state all come from this walk.
MXY_UNESC_HD uint32_t tail_code(const uint32_t (&tail)[16], uint32_t from, uint32_t e0) {
    uint32_t code = 0;
    for (uint32_t s = 0; s < 2u; ++s) {
        uint32_t e = (e0 >> s) & 1u, six = 0;
        MXY_UNESC_UNROLL
        for (uint32_t k = 0; k < 16u; ++k) {
            if (k >= 10u) six |= e << (k - 10u);
            if (k >= from) e = (tail[k] == '\\') & (e ^ 1u);
        }
        code |= (e | (six << 1)) << (8u * s);
    }
    return code;
}

MXY_UNESC_HD uint64_t tiles(uint64_t len) { return (len + TILE_BYTES - 1) / TILE_BYTES; }

// ---- CPU driver: the passes over one tile, the way the kernels partition the work ----------------------------------------------------
struct Counters { uint64_t escapes = 0, replaced = 0, lf_escapes = 0; };

// The code of full tile t ((t + 1) * TILE_BYTES <= len): the backslash run in front of byte 10 of the tile's last 16 is followed back to
// its first byte or to the tile's, as the kernel does.
inline uint32_t tile_state_code(const uint8_t* data, size_t len, uint64_t t) {
    (void)len;
    const uint8_t* tile = data + t * TILE_BYTES;
    uint32_t tail[16];
    for (uint32_t k = 0; k < 16u; ++k) tail[k] = tile[TILE_BYTES - 16 + k];
    for (int k = 9; k >= 0; --k)
        if (tail[k] != '\\') return tail_code(tail, (uint32_t)k + 1u, 0u);
    uint32_t run = 0;   // backslashes in front of the tail
    while (run < TILE_BYTES - 16 && tile[TILE_BYTES - 17 - run] == '\\') ++run;
    const uint32_t par = run & 1u;
    return tail_code(tail, 0u, run == TILE_BYTES - 16 ? (par ? 1u : 2u) : (par ? 3u : 0u));
}

// the window of lane `lane` of tile t; esc of the tile's bytes from its state (PERCENT: esc stays 0)
inline Window tile_window(const uint8_t* data, size_t len, uint32_t mode, uint64_t t, uint32_t lane, uint32_t state) {
    Window w;
    const int64_t base = (int64_t)(t * TILE_BYTES + (uint64_t)lane * LANE_BYTES);
    for (uint32_t j = 0; j < WINDOW_BYTES; ++j) {
        const int64_t i = base - (int64_t)OWN + (int64_t)j;
        w.b[j] = i >= 0 && (uint64_t)i < len ? data[i] : BYTE_NONE;
    }
    w.esc = 0;
    if (mode != MODE_JSON) return w;
    // esc of the tile's bytes in front of the lane, walked from the tile's first byte
    uint32_t e = state & 1u;
    uint32_t hist = (state >> 1) & 0x3Fu;   // esc of the six bytes in front of the walk, oldest in bit 0
    for (uint64_t i = t * TILE_BYTES; i < (uint64_t)base && i < len; ++i) {
        hist = (hist >> 1) | (e << 5);
        e = (data[i] == '\\') & (e ^ 1u);
    }
    w.esc = hist | (lane_esc(w, e) << OWN);
    return w;
}
// output bytes of tile t; *c grows by what the tile adds to the counters
inline uint32_t tile_count(const uint8_t* data, size_t len, uint32_t mode, uint64_t t, uint32_t state, Counters* c = nullptr) {
    uint32_t n = 0;
    for (uint32_t lane = 0; lane < TILE_LANES; ++lane) {
        const Window w = tile_window(data, len, mode, t, lane, state);
        for (uint32_t k = 0; k < LANE_BYTES; ++k) {
            n += item_len(w, OWN + k, mode);
            const uint32_t f = item_flags(w, OWN + k, mode);
            if (c) { c->escapes += f & F_ESCAPE ? 1 : 0; c->replaced += f & F_REPLACED ? 1 : 0; c->lf_escapes += f & F_LF ? 1 : 0; }
        }
    }
    return n;
}
// writes the bytes of tile t to out[0 ..) (room for TILE_OUT_MAX) and returns their number
inline uint32_t tile_write(const uint8_t* data, size_t len, uint32_t mode, uint64_t t, uint32_t state, uint8_t* out) {
    uint32_t n = 0;
    for (uint32_t lane = 0; lane < TILE_LANES; ++lane) {
        const Window w = tile_window(data, len, mode, t, lane, state);
        const bool lit = lane_is_literal(w, mode);   // the kernels' shortcut: it must give the same bytes
        for (uint32_t k = 0; k < LANE_BYTES; ++k) {
            if (lit) { if (w.b[OWN + k] != BYTE_NONE) out[n++] = (uint8_t)w.b[OWN + k]; continue; }
            const uint32_t l = item_len(w, OWN + k, mode);
            uint32_t b = item_bytes(w, OWN + k, mode);
            for (uint32_t j = 0; j < l; ++j, b >>= 8) out[n++] = (uint8_t)b;
        }
    }
    return n;
}

}  // namespace unescape
}  // namespace mxy
