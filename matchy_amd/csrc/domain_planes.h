// Bit-sliced label rules of k_validate_dom (host + device, so that the CPU test suite can check them exhaustively).
//
// A lane of k_validate_dom holds the context record of one domain anchor as k_anchor wrote it: eight dwords c[0..7] =
// log[j-24, j+8) in address order, j = first byte of the last label. context_planes() turns them into 32-bit class masks
// whose bit p stands for context byte p — bits 0..23 the look-back, bits 24..31 the label window — with the 8 x 8 bit
// transpose and the class functions of k_anchor (anchor_planes.h): one 32-bit operation per class term for the whole
// record, where byte-lane SWAR on 64-bit words needed eight passes of four positions each. The rules of is_valid_domain
// (ext:637-689) then are shifts, counts and bit tests on those masks (domain_rules()).
//
// Bit order. bit_transpose8() leaves bit 8 b + q of plane k = bit k of byte b of word q, so the masks come out in address
// order if byte b of word q is context byte 8 b + q: a 4 x 4 byte transpose of the even dwords (q = 0..3) and of the odd
// ones (q = 4..7) in FRONT of the bit transpose, two rounds of v_perm_b32, 16 in all. The other way round — transposing
// the dwords as they are and putting the bits of each class mask in order BEHIND it — moves bit 8 b + q to bit 4 q + b: a
// rotation of the five index bits by two, i.e. four delta swaps (six operations each) per mask, and there are five masks:
// 120 operations against 16. The gather in front is the one used.
#pragma once
#include <cstdint>

#include "anchor_planes.h"

namespace mxy {

// bytes sel[k] (0..3: of lo, 4..7: of hi) of the eight bytes hi:lo, k = 0..3 (v_perm_b32; selectors above 7 are not used here)
MXY_HD uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7u))) & 0xFFu) << (8 * k);
    return r;
#endif
}

struct ContextMasks {
    uint32_t DC;     // DOMAIN_CHAR_LOOKUP (ext:1597-1629): letter, digit, '.', '-', byte >= 0x80
    uint32_t DOT;    // '.'
    uint32_t DASH;   // '-'
    uint32_t HIGH;   // byte >= 0x80
    uint32_t B;      // boundary byte (BOUNDARY_LOOKUP, ext:1568-1593)
};

// c[i] = context bytes [4 i, 4 i + 4). Bit p of every mask = context byte p.
MXY_HD ContextMasks context_planes(const uint32_t (&c)[8]) {
    uint32_t w[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // words h, h + 2, h + 4, h + 6 -> w[4 h + q] = their bytes q
        const uint32_t alo = byte_perm(c[h + 2], c[h], 0x05010400u), ahi = byte_perm(c[h + 2], c[h], 0x07030602u);
        const uint32_t blo = byte_perm(c[h + 6], c[h + 4], 0x05010400u), bhi = byte_perm(c[h + 6], c[h + 4], 0x07030602u);
        w[4 * h + 0] = byte_perm(blo, alo, 0x05040100u);
        w[4 * h + 1] = byte_perm(blo, alo, 0x07060302u);
        w[4 * h + 2] = byte_perm(bhi, ahi, 0x05040100u);
        w[4 * h + 3] = byte_perm(bhi, ahi, 0x07060302u);
    }
    bit_transpose8(w);
    // the wide form of TL is "label byte or '-'": with the dot it is the domain-char class, without the label bytes the dash
    const ClassPlanes k = classify_planes(w, true);
    ContextMasks m;
    m.DC = k.TL | k.T;
    m.DOT = k.T;
    m.DASH = andn(k.LD, k.TL);
    m.HIGH = w[7];
    m.B = k.B;
    return m;
}

MXY_HD uint32_t dp_ctz(uint32_t x) { return (uint32_t)__builtin_ctz(x); }   // x != 0
MXY_HD uint32_t dp_clz(uint32_t x) { return (uint32_t)__builtin_clz(x); }   // x != 0
MXY_HD uint32_t dp_popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// The domain anchor at j with its context record, decided from the masks where that is possible: last label of <= 7 bytes
// that alone is a public suffix, name no longer than the look-back. `tldtab`: the exact table of last labels (DevDb::tld_tab;
// Slot = uint2 or anything with x and y), 1 << TLD_TAB_BITS slots.
// `pfxtab`: the exact table of the 8-byte windows that start a last label of 8 bytes or more (DevDb::tld_pfx, hashes.h), or
// null. With it a window of 8 label bytes that starts no such label is no domain — what k_anchor's Bloom filter let through by mistake
// ends here and not in the general walk; without it every such window is undecided.
// Returns 0 (no domain), 1 (domain: start / end set, the whole name lies in the context) or 2 (undecided: general path).
template <class Slot, class PfxSlot>
MXY_HD int domain_rules(const Slot* tldtab, const PfxSlot* pfxtab, uint32_t min_labels, uint32_t j, const uint32_t (&c)[8], uint32_t& start,
                        uint32_t& end) {
    const ContextMasks m = context_planes(c);
    // last label = the domain-char bytes from bit 24 up; ll = its length (8: not terminated within the window)
    const uint32_t ndc = ~m.DC >> 24;
    const uint32_t ll = ndc ? dp_ctz(ndc) : 8u;
    const uint32_t label = ((1u << ll) - 1u) << 24;                  // the label's bits
    // What the masks say about the run in front of the label, for every record and without a branch: nearly every record is a genuine
    // name that needs all of it, and an early way out is a pair of scalar instructions on the exec mask per test for nothing.
    // The run extends downwards from bit 23 (the dot at j-1) while bytes are domain chars; the low byte of ~(DC << 8) is set: <= 24
    const uint32_t consumed = dp_clz(~(m.DC << 8));
    const uint32_t li = 24 - consumed;                               // leftmost byte of the run
    const uint32_t r = (0xFFFFFFFFu << li) & 0x00FFFFFFu;            // the run's bits
    const uint32_t D = m.DOT & 0x00FFFFFFu, S = m.DASH & 0x00FFFFFFu;
    // bad events, seen from the left byte of a pair: empty label (dot, dot), label starting with '-' (dot, dash), label ending with '-'
    // (dash, dot). Right of bit 23 stands the label's first byte, which is neither.
    const uint32_t bad = ((D & ((D | S) >> 1)) | (S & (D >> 1))) & r;
    const uint32_t ndots = dp_popc(D & r);
    // the leftmost byte must not be a dot (empty leftmost label) or a dash, the label's last byte not a dash
    const uint32_t edge = (((D | S) >> li) | (m.DASH >> (23 + ll))) & 1u;
    const uint32_t front = ((m.B << 1) >> li) & 1u;                  // the byte in front of the run is a boundary (bit li - 1; none at li = 0)
    const bool whole = consumed == 24;                               // the run fills the look-back: a name only if the buffer starts here
    const bool no_name = ((bad | edge) != 0) | (consumed == 0) | (ndots == 0) | (1 + ndots < min_labels) | (!whole & (front == 0));
    const bool high = (m.HIGH & (r | label)) != 0;                   // needs the UTF-8 check of the general path
    const int by_run = (whole & (j != 24)) ? 2 : no_name ? 0 : high ? 2 : 1;
    const bool no_label = ((m.DOT & label) != 0) | ((((m.B >> 24) >> ll) & 1u) == 0);   // a later dot owns this run; the stop byte
    if (ll < 1) return 2;
    if (ll > 7) return (pfxtab == nullptr || tld_pfx_has(pfxtab, c[6], c[7])) ? 2 : 0;
    if (no_label) return 0;
    const uint32_t lo = ll >= 4 ? c[6] : c[6] & ((1u << (8 * ll)) - 1u);
    const uint32_t hi = ll > 4 ? c[7] & ((1u << (8 * ll - 32)) - 1u) : 0u;
    uint32_t slot = tld_tab_slot(lo, hi);
    bool alone = false;
    for (;;) {
        const Slot t = tldtab[slot];
        if ((t.y >> 24) == 0) return 0;
        if (t.x == lo && (t.y & 0xFFFFFFu) == hi) { alone = (t.y >> 24) & 1; break; }
        slot = (slot + 1) & ((1u << TLD_TAB_BITS) - 1);
    }
    if (!alone) return 2;
    start = j - consumed; end = j + ll;
    return by_run;
}
template <class Slot>
MXY_HD int domain_rules(const Slot* tldtab, uint32_t min_labels, uint32_t j, const uint32_t (&c)[8], uint32_t& start, uint32_t& end) {
    return domain_rules(tldtab, (const Slot*)nullptr, min_labels, j, c, start, end);
}

}  // namespace mxy
