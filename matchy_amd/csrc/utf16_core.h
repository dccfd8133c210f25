// UTF-16 -> UTF-8: the one definition of the transcoding, for the kernels (utf16.hip) and for a CPU driver (tests). Host and device;
// the host needs no HIP include.
//
// The input is `len` bytes read as len / 2 16-bit code units in the given byte order; an odd last byte is one more item behind them.
// Item i of the input is a code unit, UNIT_ODD (the odd last byte) or UNIT_NONE (in front of the input or behind it), and what an item
// turns into depends on itself and its two neighbours alone:
//   x < 0x80                          1 byte
//   x < 0x800                         2 bytes
//   high surrogate, next is low       the 4 bytes of the pair's code point
//   low surrogate, prev is high       0 bytes (the high one wrote them)
//   any other surrogate, UNIT_ODD     EF BF BD (U+FFFD: one per item, the rule of Rust's String::from_utf16_lossy)
//   every other unit                  3 bytes
//   UNIT_NONE                         0 bytes
// `high high low` is one U+FFFD and one pair, `low low` two U+FFFD, and a high surrogate in front of the odd byte is unpaired (CPython's
// codec merges those two into one U+FFFD; this one does not). No BOM handling: U+FEFF becomes EF BB BF, U+FFFE becomes EF BF BE.
// unit_len and unit_bytes are the only place where the length of an item and its bytes are decided: a count pass and a write pass that
// are both built from them cannot disagree.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MXY_UTF16_HD __host__ __device__ __forceinline__
#else
#define MXY_UTF16_HD inline
#endif

namespace mxy {
namespace utf16 {

constexpr uint32_t ORDER_LE = 0, ORDER_BE = 1;
constexpr uint32_t UNIT_NONE = 0xFFFFFFFFu;   // no item: in front of the input or behind it
constexpr uint32_t UNIT_ODD = 0x00010000u;    // the odd last byte
// Work partition of the passes: a tile is TILE_BYTES input bytes = TILE_UNITS items, and gives at most TILE_OUT_MAX bytes: three per
// item, and one more where the tile's last unit is a high surrogate whose low one opens the next tile (which then gives three less)
constexpr uint32_t TILE_BYTES = 1024, TILE_UNITS = TILE_BYTES / 2, TILE_OUT_MAX = 3 * TILE_UNITS + 1;

MXY_UTF16_HD bool is_high(uint32_t x) { return (x & 0xFFFFFC00u) == 0xD800u; }
MXY_UTF16_HD bool is_low(uint32_t x) { return (x & 0xFFFFFC00u) == 0xDC00u; }
// the item is written as U+FFFD
MXY_UTF16_HD bool unit_replaced(uint32_t prev, uint32_t x, uint32_t next) {
    if (x == UNIT_ODD) return true;
    if (is_high(x)) return !is_low(next);
    if (is_low(x)) return !is_high(prev);
    return false;
}
MXY_UTF16_HD uint32_t unit_len(uint32_t prev, uint32_t x, uint32_t next) {
    if (x == UNIT_NONE) return 0;
    if (x < 0x80u) return 1;
    if (x < 0x800u) return 2;
    if (is_high(x) && is_low(next)) return 4;
    if (is_low(x) && is_high(prev)) return 0;
    return 3;
}
// the unit_len(prev, x, next) bytes of the item, first byte in bits 0..7
MXY_UTF16_HD uint32_t unit_bytes(uint32_t prev, uint32_t x, uint32_t next) {
    if (x == UNIT_NONE) return 0;
    if (x < 0x80u) return x;
    if (x < 0x800u) return (0xC0u | (x >> 6)) | ((0x80u | (x & 0x3Fu)) << 8);
    if (is_high(x) && is_low(next)) {
        const uint32_t c = 0x10000u + ((x & 0x3FFu) << 10) + (next & 0x3FFu);
        return (0xF0u | (c >> 18)) | ((0x80u | ((c >> 12) & 0x3Fu)) << 8) | ((0x80u | ((c >> 6) & 0x3Fu)) << 16) | ((0x80u | (c & 0x3Fu)) << 24);
    }
    if (is_low(x) && is_high(prev)) return 0;
    if (unit_replaced(prev, x, next)) return 0x00BDBFEFu;
    return (0xE0u | (x >> 12)) | ((0x80u | ((x >> 6) & 0x3Fu)) << 8) | ((0x80u | (x & 0x3Fu)) << 16);
}

// upper bound of the output of `len` input bytes
MXY_UTF16_HD uint64_t out_bound(uint64_t len) { return 3u * (len / 2) + 3u * (len & 1u); }
MXY_UTF16_HD uint64_t tiles(uint64_t len) { return (len + TILE_BYTES - 1) / TILE_BYTES; }

// ---- CPU driver: the passes over one tile, the way the kernels partition the work ----------------------------------------------------
// item i of the input (i may be -1 or lie behind the input)
inline uint32_t item_at(const uint8_t* data, size_t len, uint32_t order, int64_t i) {
    const int64_t n_units = (int64_t)(len / 2);
    if (i < 0 || i > n_units) return UNIT_NONE;
    if (i == n_units) return (len & 1u) ? UNIT_ODD : UNIT_NONE;
    const uint32_t a = data[2 * i], b = data[2 * i + 1];
    return order == ORDER_BE ? (a << 8) | b : (b << 8) | a;
}
// output bytes of tile `t`; *replaced grows by the U+FFFD it writes
inline uint32_t tile_count(const uint8_t* data, size_t len, uint32_t order, uint64_t t, uint64_t* replaced = nullptr) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < TILE_UNITS; ++k) {
        const int64_t i = (int64_t)(t * TILE_UNITS + k);
        const uint32_t p = item_at(data, len, order, i - 1), x = item_at(data, len, order, i), q = item_at(data, len, order, i + 1);
        n += unit_len(p, x, q);
        if (replaced && x != UNIT_NONE && unit_replaced(p, x, q)) ++*replaced;
    }
    return n;
}
// writes the bytes of tile `t` to out[0 ..) (room for TILE_OUT_MAX) and returns their number
inline uint32_t tile_write(const uint8_t* data, size_t len, uint32_t order, uint64_t t, uint8_t* out) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < TILE_UNITS; ++k) {
        const int64_t i = (int64_t)(t * TILE_UNITS + k);
        const uint32_t p = item_at(data, len, order, i - 1), x = item_at(data, len, order, i), q = item_at(data, len, order, i + 1);
        const uint32_t l = unit_len(p, x, q);
        uint32_t b = unit_bytes(p, x, q);
        for (uint32_t j = 0; j < l; ++j, b >>= 8) out[n++] = (uint8_t)b;
    }
    return n;
}

}  // namespace utf16
}  // namespace mxy
