// The label-window rule of k_anchor's domain drain and the exact table of long-label prefixes behind it (host + device, so that the
// CPU test suite can check both against the shipped public-suffix list).
//
// A domain anchor is the first byte j of a label behind a dot; the drain holds log[j, j + 8), the label window. A label can only be
// the LAST label of a name if some public suffix ends with it (val_domain, validate_kernels.hip: "last label is no suffix's last
// label -> no PSL hit possible"), and the list is fixed per database. So the window decides every label, long ones included:
//   label ends inside the window (ll <= 7)  -> no dot in it, a boundary byte behind it, the label in the filter
//   window full of domain characters (ll = 8) -> no dot in it, the WINDOW in the filter: it is either a last label of exactly 8 bytes
//                                               or the first 8 bytes of a longer one, and the filter holds both kinds of key
// with one straight line of code for both (label_window_keep). The filter is k_anchor's own Bloom filter (two bits per key, built in
// load_psl, engine.cpp); what it lets through by mistake ends in k_validate_dom, which asks an exact table (tld_pfx_*, hashes.h) for
// windows of 8 label bytes and the exact table of short labels (DevDb::tld_tab) for the rest.
//
// Accepted: a long MIDDLE label whose first 8 bytes are such a key ("www.microsoft.com", "www.americanexpress.com") passes both — 8 bytes
// do not show the dot behind them — and is refused by the general walk ("a later dot owns the run").
#pragma once
#include <cstdint>

#include "hashes.h"

namespace mxy {

// Byte-class masks of 8 log bytes at once (SWAR; bit 7 of each byte of the result is the class bit, all other bits 0).
// Every addend keeps each byte below 0x100, so no carry crosses a byte.
struct ByteMasks { uint64_t dc, dot, dash, high; };
// The class arithmetic keeps every byte lane below 0x100, so no carry ever crosses a byte — nor the middle of a 64-bit word: the two
// halves are computed on their own with 32-bit adds. (Written on uint64_t the compiler emits v_add_co / v_addc_co pairs, a carry chain
// through VCC that costs twice as much on the vector pipe; it also fuses a 64-bit expression that merely spells the two halves back
// into that form, hence the separate function.)
struct ByteMasks32 { uint32_t dc, dot, dash, high; };
MXY_HD ByteMasks32 domain_masks32(uint32_t x) {
    constexpr uint32_t H = 0x80808080u, L7 = 0x7F7F7F7Fu;
    const uint32_t t = x & L7, l = t | 0x20202020u;
    const uint32_t dig = (t + 0x50505050u) & ~(t + 0x46464646u);   // '0'..'9'
    const uint32_t alp = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u);   // 'a'..'z' after case folding
    const uint32_t ndot = (t ^ 0x2E2E2E2Eu) + L7, ndash = (t ^ 0x2D2D2D2Du) + L7;  // bit 7 set iff different
    ByteMasks32 m;
    m.high = x & H;
    m.dot = ~ndot & ~x & H;
    m.dash = ~ndash & ~x & H;
    m.dc = (((dig | alp) & ~x) | m.dot | m.dash | m.high) & H;  // DOMAIN_CHAR_LOOKUP (ext:1597-1629)
    return m;
}
MXY_HD ByteMasks domain_masks(uint64_t x) {
    const ByteMasks32 lo = domain_masks32((uint32_t)x), hi = domain_masks32((uint32_t)(x >> 32));
    ByteMasks m;
    m.dc = (uint64_t)lo.dc | ((uint64_t)hi.dc << 32);
    m.dot = (uint64_t)lo.dot | ((uint64_t)hi.dot << 32);
    m.dash = (uint64_t)lo.dash | ((uint64_t)hi.dash << 32);
    m.high = (uint64_t)lo.high | ((uint64_t)hi.high << 32);
    return m;
}

// bits of the prefilter's Bloom filter (half of TLD_BLOOM_BITS, scan_types.h): a key sets bits 0..13 and 14..27 of tld_hash8
constexpr uint32_t TLD_PREFILTER_BITS = 1u << 14;

// Keep (true) or drop the resident domain anchor whose label window is hi:lo = log[j, j + 8), little-endian. `filter`: the
// TLD_PREFILTER_BITS bits of the prefilter's Bloom filter; is_boundary(byte): BOUNDARY_LOOKUP. No branch on the label length: with no
// non-domain byte in the window ll is 8, `below` is all ones, the key is the whole window and the stop-byte test is skipped; a dot
// anywhere in such a window drops it through the same (dot & below) term that finds a dot inside a short label.
// Never drops an anchor that val_domain accepts; keeps what the filter lets through by mistake and long middle labels (see above).
template <class Boundary>
MXY_HD bool label_window_keep(uint32_t lo, uint32_t hi, const uint32_t* filter, Boundary is_boundary) {
    constexpr uint32_t H = 0x80808080u;
    const ByteMasks32 ml = domain_masks32(lo), mh = domain_masks32(hi);
    const uint32_t nl = ~ml.dc & H, nh = ~mh.dc & H;                 // bit 7 of the bytes that are no domain characters
    // bit 8 ll of the window, ll = the label's length; none when the window is full. One below it are the label's own bits.
    const uint32_t el = (nl & (0u - nl)) >> 7, eh = nl ? 0u : (nh & (0u - nh)) >> 7;
    const uint32_t bl = el - 1u, bh = nl ? 0u : eh - 1u;             // `below`, in halves (32-bit: no carry chain)
    const bool full = (nl | nh) == 0;
    const uint32_t at = nl ? (uint32_t)__builtin_ctz(nl) - 7u : (uint32_t)__builtin_ctz(nh | 0x80000000u) - 7u;
    const uint32_t stop = ((nl ? lo : hi) >> at) & 0xFFu;            // the byte behind the label (a label byte when the window is full)
    const uint32_t h8 = tld_hash8(lo & bl, hi & bh);
    const uint32_t b1 = h8 & (TLD_PREFILTER_BITS - 1), b2 = (h8 >> 14) & (TLD_PREFILTER_BITS - 1);
    const uint32_t in_filter = (filter[b1 >> 5] >> (b1 & 31)) & (filter[b2 >> 5] >> (b2 & 31)) & 1u;
    // a '.' inside the label: a later dot owns the run; the run must end at a boundary; the label (or its first 8 bytes) must be (those
    // of) some public suffix's last label
    return (((ml.dot & bl) | (mh.dot & bh)) == 0) & (full | is_boundary(stop)) & (in_filter != 0);
}

// host (load_psl, engine.cpp): enter the last label of a public suffix, ll >= 1 bytes at `last`, into the prefilter's filter — with what
// the window shows of it: all of it up to 8 bytes, else its first 8 — and a window of 8 label bytes into the exact table `pfx`
// (1 << TLD_PFX_BITS slots, hashes.h) as well. Returns true if that window is new to the table.
template <class Slot>
inline bool prefilter_add_label(uint32_t* filter, Slot* pfx, const uint8_t* last, size_t ll) {
    uint8_t k8[8] = {0};
    for (size_t k = 0; k < ll && k < 8; ++k) k8[k] = last[k];
    const uint32_t lo = k8[0] | (uint32_t)k8[1] << 8 | (uint32_t)k8[2] << 16 | (uint32_t)k8[3] << 24;
    const uint32_t hi = k8[4] | (uint32_t)k8[5] << 8 | (uint32_t)k8[6] << 16 | (uint32_t)k8[7] << 24;
    const uint32_t h8 = tld_hash8(lo, hi);
    const uint32_t b1 = h8 & (TLD_PREFILTER_BITS - 1), b2 = (h8 >> 14) & (TLD_PREFILTER_BITS - 1);
    filter[b1 >> 5] |= 1u << (b1 & 31);
    filter[b2 >> 5] |= 1u << (b2 & 31);
    return ll >= 8 && tld_pfx_insert(pfx, lo, hi);
}

}  // namespace mxy
