// Bit-sliced front end of k_anchor (host + device, so that the CPU test suite can check it exhaustively).
//
// A wavefront stages 2 KiB of log per block as 8 rows of 256 bytes: lane L holds dword L of every row, w[q] = bytes
// [256 q + 4 L, 256 q + 4 L + 4) of the block. bit_transpose8() turns the lane's 8 dwords into the 8 bit planes of its 32
// bytes: afterwards bit (8 b + q) of w[c] is bit c of byte b of row q. classify_planes() evaluates the byte classes of
// the extractor (reference: BOUNDARY_LOOKUP matchy-extractor/src/lib.rs:1568-1593, DOMAIN_CHAR_LOOKUP :1597-1629) as
// boolean functions of those planes — one 32-bit operation handles 32 log positions per lane, where byte-lane SWAR on
// class bytes handled 4 — and the anchor patterns then need nothing but shifted copies of the class planes:
// "the byte k positions earlier" is v_alignbyte(P, P_of_previous_dword, 4 - k), because consecutive dwords of a row sit in
// consecutive lanes with the same bit layout.
#pragma once
#include <cstdint>

#include "hashes.h"   // MXY_HD

namespace mxy {

struct ClassPlanes {
    uint32_t B;    // boundary byte (20 byte values)
    uint32_t D;    // '0'..'9'
    uint32_t T;    // '.'
    uint32_t C;    // ':'
    uint32_t AT;   // '@'
    uint32_t NL;   // '\n'
    uint32_t LD;   // label byte: alphanumeric or >= 0x80
    uint32_t TL;   // may start the last label of a public suffix (superset: 'a'..'z' or >= 0x80; wide mode: any label byte or '-')
};

// (x & m) | (y & ~m): v_bfi_b32
MXY_HD uint32_t bsel(uint32_t m, uint32_t x, uint32_t y) { return (x & m) | (y & ~m); }
// y & ~m
MXY_HD uint32_t andn(uint32_t m, uint32_t y) { return y & ~m; }

// 8 x 8 bit-matrix transpose of the four byte lanes of w[0..7] at once (three butterfly stages, v_lshl/v_lshr + v_bfi). In two parts
// for k_anchor: the first stage reads the registers the block was loaded into and writes new ones, so the loads of the next block can be
// issued into the old ones right behind it — with the whole transpose in place the block first had to be copied out of their way
// (8 moves per block, and 4 wide ones back on the path without a next block).
#define MXY_SWAP(a, b, s, m) { const uint32_t ta = bsel(m, w[a], w[b] << s), tb = bsel(m, w[a] >> s, w[b]); w[a] = ta; w[b] = tb; }
MXY_HD void bit_transpose8_first(const uint32_t (&in)[8], uint32_t (&w)[8]) {
#pragma unroll
    for (int a = 0; a < 8; a += 2) {
        w[a] = bsel(0x55555555u, in[a], in[a + 1] << 1);
        w[a + 1] = bsel(0x55555555u, in[a] >> 1, in[a + 1]);
    }
}
MXY_HD void bit_transpose8_rest(uint32_t (&w)[8]) {
    MXY_SWAP(0, 2, 2, 0x33333333u) MXY_SWAP(1, 3, 2, 0x33333333u) MXY_SWAP(4, 6, 2, 0x33333333u) MXY_SWAP(5, 7, 2, 0x33333333u)
    MXY_SWAP(0, 4, 4, 0x0F0F0F0Fu) MXY_SWAP(1, 5, 4, 0x0F0F0F0Fu) MXY_SWAP(2, 6, 4, 0x0F0F0F0Fu) MXY_SWAP(3, 7, 4, 0x0F0F0F0Fu)
}
#undef MXY_SWAP
MXY_HD void bit_transpose8(uint32_t (&w)[8]) {
    uint32_t t[8];
    bit_transpose8_first(w, t);
    bit_transpose8_rest(t);
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = t[q];
}

// The boundary class alone (classify_planes().B): 09 0A 0D | 20 22 27 28 29 2C 2F | 3A 3B 3C 3D 3E | 40 | 5B 5D 7B 7D. It is the
// most expensive class (21 vector instructions in k_anchor's gfx950 code: the basic block that evaluates it on top of the other
// classes, three-input v_bitop3 included) and only the long-token code reads it, so k_anchor
// evaluates it where that code needs it (see "Long tokens" below) and not in every block.
MXY_HD uint32_t boundary_plane(const uint32_t (&p)[8]) {
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7];
    const uint32_t o76 = p7 | p6;
    const uint32_t a5 = andn(o76, p5);          // 0x20..0x3F
    const uint32_t h3 = a5 & p4;                // 0x30..0x3F
    const uint32_t h2 = andn(p4, a5);           // 0x20..0x2F
    const uint32_t o54 = p5 | p4;
    const uint32_t o7654 = o76 | o54;           // clear: 0x00..0x0F
    const uint32_t b = andn(p7, p6);            // 0x40..0x7F
    const uint32_t h4 = andn(o54, b);           // 0x40..0x4F
    const uint32_t b4 = b & p4;                 // 0x50..0x5F, 0x70..0x7F
    const uint32_t a10 = p1 & p0, o10 = p1 | p0, x10 = p1 ^ p0;
    const uint32_t o3210 = (p3 | p2) | o10;     // clear: low nibble 0
    const uint32_t g9 = p3 & (p2 | p1);         // low nibble > 9
    const uint32_t at = andn(o3210, h4);                                        // 0x40
    const uint32_t B0 = andn(o7654, p3 & andn(p2 & p1, x10));                   // low nibble 9, A, D
    const uint32_t f2 = bsel(p3, bsel(p2, ~x10, ~p1), bsel(p2, a10, ~p0));      // low nibble 0, 2, 7, 8, 9, C, F
    const uint32_t B2 = h2 & f2;
    const uint32_t B3 = andn(p2 & a10, h3 & g9);                                // 3A..3E
    const uint32_t B57 = b4 & (p3 & p0) & (p2 ^ p1);                            // low nibble B, D
    return B0 | B2 | B3 | at | B57;
}

// Byte classes from the bit planes p[0] (bit 0 of every byte) .. p[7]. `tl_wide`: the public-suffix list in use has a last
// label that starts with something other than 'a'..'z' / a byte >= 0x80 (never the case for the shipped list): then every
// byte that can be part of a label counts as a possible first byte.
MXY_HD ClassPlanes classify_planes(const uint32_t (&p)[8], bool tl_wide) {
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4], p5 = p[5], p6 = p[6], p7 = p[7];
    // high nibble
    const uint32_t o76 = p7 | p6;
    const uint32_t a5 = andn(o76, p5);          // 0x20..0x3F
    const uint32_t h3 = a5 & p4;                // 0x30..0x3F
    const uint32_t h2 = andn(p4, a5);           // 0x20..0x2F
    const uint32_t o54 = p5 | p4;
    const uint32_t o7654 = o76 | o54;           // clear: 0x00..0x0F
    const uint32_t b = andn(p7, p6);            // 0x40..0x7F
    const uint32_t h4 = andn(o54, b);           // 0x40..0x4F
    // low nibble terms
    const uint32_t a10 = p1 & p0, o10 = p1 | p0;
    const uint32_t a32 = p3 & p2, o32 = p3 | p2;
    const uint32_t o3210 = o32 | o10;           // clear: low nibble 0
    ClassPlanes c;
    c.T = h2 & andn(p0, a32 & p1);                          // 0x2E
    const uint32_t g9 = p3 & (p2 | p1);                     // low nibble > 9
    c.D = andn(g9, h3);                                     // 0x30..0x39
    const uint32_t loA = andn(p2 | p0, p3 & p1);            // low nibble == 0xA
    c.NL = andn(o7654, loA);                                // 0x0A
    c.C = h3 & loA;                                         // 0x3A
    c.AT = andn(o3210, h4);                                 // 0x40
    // letters: 0x41..0x4F / 0x61..0x6F (p4 clear, low nibble != 0), 0x50..0x5A / 0x70..0x7A (p4 set, low nibble <= 0xA)
    const uint32_t gA = p3 & (p2 | a10);                    // low nibble > 0xA
    const uint32_t not_letter = bsel(p4, gA, ~o3210);
    const uint32_t alpha = andn(not_letter, b);
    c.LD = alpha | c.D | p7;
    c.B = boundary_plane(p);   // shares its nibble terms with the classes above (common subexpressions); dropped where nobody reads it
    c.TL = tl_wide ? (c.LD | (h2 & a32 & andn(p1, p0))) : ((alpha & p5) | p7);  // wide: label byte or '-' (0x2D)
    return c;
}

// Row/lane geometry of a block
constexpr uint32_t AB_ROWS = 8, AB_ROW_BYTES = 256, AB_BLOCK = AB_ROWS * AB_ROW_BYTES;
// offset inside the block of the position that bit t of lane `lane` stands for
MXY_HD uint32_t plane_bit_offset(uint32_t lane, uint32_t t) { return ((t & 7u) << 8) + (lane << 2) + (t >> 3); }

// ---- shifted planes. PV / NV = the plane word of the previous / next dword of the byte stream (lane L-1 / L+1; across the
// ends of a row: the neighbouring row of lane 63 / lane 0, see plane_prev_dword / plane_next_dword in k_anchor.hip).
// bytes k .. k+3 of the eight bytes hi:lo (v_alignbyte_b32)
MXY_HD uint32_t plane_alignbyte(uint32_t hi, uint32_t lo, uint32_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, k);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * k));
#endif
}
// class of the byte K positions earlier / later (K = 1..4), aligned to this position
template <int K> MXY_HD uint32_t plane_back(uint32_t P, uint32_t PV) { return K == 4 ? PV : plane_alignbyte(P, PV, 4 - K); }
template <int K> MXY_HD uint32_t plane_ahead(uint32_t P, uint32_t NV) { return K == 4 ? NV : plane_alignbyte(NV, P, K); }

// ---- IPv4 anchors
// "Neither a digit nor '.'": what may stand in front of the first octet as far as the streaming pass is concerned. It contains the
// boundary class (no boundary byte is a digit or a dot), costs one operation on planes the kernel has anyway, and the drain checks
// the byte in front of the octet exactly. The '.' stays excluded: otherwise the second and third dot of every address were anchors.
MXY_HD uint32_t nondigit_nondot_plane(uint32_t D, uint32_t T) { return ~(D | T); }
// '.' at j, a digit at j-1 (Dm1 = the digit plane one position back), a byte that is neither digit nor dot 2..4 positions back and a
// second dot 2..4 positions ahead. A superset of the dots that open a dotted quad: the drain checks the digits in between, and what
// stands at j+1 is left to it as well (on logs "digit at j+1" removed no anchor at all and cost a cross-lane move of the digit plane).
MXY_HD uint32_t ipv4_anchor_plane(uint32_t T, uint32_t Dm1, uint32_t N, uint32_t PV_N, uint32_t NV_T) {
    const uint32_t lookback = Dm1 & (plane_back<2>(N, PV_N) | plane_back<3>(N, PV_N) | plane_back<4>(N, PV_N));
    const uint32_t lookahead = plane_ahead<2>(T, NV_T) | plane_ahead<3>(T, NV_T) | plane_ahead<4>(T, NV_T);
    return T & lookback & lookahead;
}

// ---- Long tokens (>= 26 ASCII letters and digits in front of a boundary byte)
// One bit per dword: a4 bit q = "all four bytes of this lane's dword of row q are ASCII alphanumerics". A token of >= 26 such bytes
// that ends in dword i makes the dwords i-1 .. i-5 of the byte stream all-alphanumeric; dword i-1 of (row q, lane 0) is (row q-1, lane 63),
// and of (row 0, lane 0) the last dword of the previous block.
MXY_HD uint32_t tok_a4(uint32_t LD, uint32_t p7) {
    const uint32_t an = LD & ~p7;           // ASCII alphanumeric bytes
    const uint32_t t = an & (an >> 8);      // folded in two steps: bytes 0&1 / 2&3, then both halves
    return t & (t >> 16) & 0xFFu;
}
// The word that travels through the wave: bit q + 1 = row q of this lane, bit 0 = row 7 of the previous block (`aprev` = that block's
// a4 >> 7, the form in which the block loop keeps it). A word that goes from lane 63 to lane 0 moves one row up: tok_up().
MXY_HD uint32_t tok_rows(uint32_t a4, uint32_t aprev) { return (a4 << 1) | aprev; }
MXY_HD uint32_t tok_up(uint32_t v, uint32_t lanes_wrapped) { return v << lanes_wrapped; }   // lanes_wrapped: 1 in the lanes the word reached from the row below

// Reference forms over a whole block (what the wave computes with DPP / ds_bpermute): a4[L], aprev[L] as above for the 64 lanes.
// w4[L]: bit q + 1 = the dwords L-3 .. L of row q (stream order, wrapping as described) are all-alphanumeric; two lane fetches
// (one lane down, then two lanes down) instead of three.
MXY_HD void tok_windows4(const uint32_t (&a4)[64], const uint32_t (&aprev)[64], uint32_t (&w4)[64]) {
    uint32_t x[64], t[64];
    for (int L = 0; L < 64; ++L) x[L] = tok_rows(a4[L], aprev[L]);
    for (int L = 0; L < 64; ++L) t[L] = x[L] & tok_up(x[(L + 63) & 63], L < 1);
    for (int L = 0; L < 64; ++L) w4[L] = t[L] & tok_up(t[(L + 62) & 63], L < 2);
}
// (a) the cheap NECESSARY condition for "some lane has five all-alphanumeric dwords directly below it": five consecutive dwords
// i-5 .. i-1 contain the two four-dword windows that end at i-2 and at i-1, and those two dwords sit in neighbouring lanes (lane 63 and
// lane 0 are neighbours; the row does not matter for a necessary condition). So: some lane and the next one both hold a window in some row.
// A run of exactly four dwords has one window and does not fire. Wave: 6 vector instructions, one ds_bpermute, the rest scalar.
MXY_HD bool tok_trigger_from_lanes(uint64_t lanes_with_window) {
    return (lanes_with_window & ((lanes_with_window << 1) | (lanes_with_window >> 63))) != 0;
}
MXY_HD bool tok_trigger(const uint32_t (&a4)[64], const uint32_t (&aprev)[64]) {
    uint32_t w4[64];
    tok_windows4(a4, aprev, w4);
    uint64_t m = 0;
    for (int L = 0; L < 64; ++L) m |= (uint64_t)(w4[L] != 0) << L;
    return tok_trigger_from_lanes(m);
}
// (b) the exact chain: r[L] bit q + 1 = the five dwords below dword L of row q are all-alphanumeric (five single-lane steps). Bit 0
// (about the previous block) and bits above 8 carry nothing: tok_chain_rows() is the part that counts.
MXY_HD void tok_chain5(const uint32_t (&a4)[64], const uint32_t (&aprev)[64], uint32_t (&r)[64]) {
    uint32_t x[64], y[64];
    for (int L = 0; L < 64; ++L) { x[L] = tok_rows(a4[L], aprev[L]); r[L] = 0xFFFFFFFFu; }
    for (int k = 0; k < 5; ++k) {
        for (int L = 0; L < 64; ++L) y[L] = tok_up(x[(L + 63) & 63], L < 1);
        for (int L = 0; L < 64; ++L) { x[L] = y[L]; r[L] &= y[L]; }
    }
}
MXY_HD uint32_t tok_chain_rows(uint32_t r) { return (r >> 1) & 0xFFu; }   // bit q = row q

}  // namespace mxy
