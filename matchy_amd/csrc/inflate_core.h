// DEFLATE (RFC 1951) decoder rules and the gzip trailer check (RFC 1952), host + device: everything that decides whether a stream is
// valid and what it decodes to lives here, so that the CPU suite can run the rules of k_gz_inflate (inflate.hip) over corrupt streams
// under a sanitizer before any of them reaches a GPU (tests/cpp/test_inflate_core.cpp drives this header sequentially).
//
// One decoder (the state of one member) turns compressed bits into TOKENS: a literal byte, a (length, distance) match or a run of stored
// bytes, each with the output position it writes. Whoever executes the tokens (a wave, or the test's loop) only copies bytes. A token
// is handed out only after its bounds are known to hold: position + length <= the member's capacity, distance <= bytes produced.
//
// Tables are canonical: count[len] codes of every length and the symbols in code order, decoded bit by bit (<= 15 turns), with a
// first-level table of FAST_BITS bits in front for the literal/length code. A code is refused the way zlib's inflate_table refuses it:
// over-subscribed always; incomplete unless it is a single code of one bit (literal/length and distance codes only).
//
// Loop bounds: the bit reader loads at most 8 bytes per refill and never at or behind `end`; a symbol takes at most 15 turns; a code
// build takes n + 15 turns and at most 2^FAST_BITS table stores (Kraft sum <= 1, checked first); the code-length loop of a dynamic
// header advances by at least one of its HLIT + HDIST <= 316 entries per turn; a batch of tokens consumes at least one input bit per
// turn of its loop or ends.
#pragma once
#include <cstdint>

#include "hashes.h"   // MXY_HD

namespace mxy {
namespace gz {

// Status of one member, bit-identical to MATCHY_GZ_* (include/matchy_amd.h). The first error in stream order ends the member; behind a
// stream that ended, the trailer checks run in the order TRUNCATED, SIZE_MISMATCH, CRC_MISMATCH, TRAILING_DATA.
enum : int32_t {
    GZ_OK = 0, GZ_BAD_HEADER = 1, GZ_TRUNCATED = 2, GZ_BAD_BLOCK = 3, GZ_BAD_CODES = 4, GZ_BAD_SYMBOL = 5, GZ_BAD_DISTANCE = 6,
    GZ_OVERFLOW = 7, GZ_SIZE_MISMATCH = 8, GZ_CRC_MISMATCH = 9, GZ_TRAILING_DATA = 10
};

constexpr uint32_t FAST_BITS = 9, FAST_SIZE = 1u << FAST_BITS;
constexpr uint32_t MAX_LENS = 320;   // HLIT + HDIST <= 286 + 30, and the 288 + 32 lengths of the fixed codes

// 2176 bytes; k_gz_inflate keeps one per wave in LDS.
struct Tables {
    uint16_t fast[FAST_SIZE];   // literal/length codes of <= FAST_BITS bits by their (bit-reversed) code: symbol << 4 | bits; 0 = none
    uint16_t len_count[16], len_sym[288];
    uint16_t dist_count[16], dist_sym[32];   // while a dynamic header is read: the code-length code
    uint16_t offs[16], next[16];             // scratch of build_code
    uint8_t lens[MAX_LENS];                  // code lengths as read
};

// Compressed bytes of one member: in[0, end). Low bits of `buf` come first; cnt of them are valid, the rest is zero.
struct BitReader {
    const uint8_t* in;
    uint32_t pos, end;
    uint64_t buf;
    uint32_t cnt;
};

MXY_HD void br_fill(BitReader& b) {
    while (b.cnt <= 56u && b.pos < b.end) { b.buf |= (uint64_t)b.in[b.pos++] << b.cnt; b.cnt += 8u; }
}
// n <= 16 bits; false: the input ends first (nothing is consumed)
MXY_HD bool br_take(BitReader& b, uint32_t n, uint32_t& v) {
    if (b.cnt < n) { br_fill(b); if (b.cnt < n) return false; }
    v = (uint32_t)b.buf & ((1u << n) - 1u);
    b.buf >>= n; b.cnt -= n;
    return true;
}
// drops the bits up to the next byte boundary and returns the position of that byte
MXY_HD uint32_t br_align(BitReader& b) {
    const uint32_t drop = b.cnt & 7u;
    b.buf >>= drop; b.cnt -= drop;
    return b.pos - b.cnt / 8u;
}
MXY_HD void br_seek(BitReader& b, uint32_t pos) { b.pos = pos; b.buf = 0; b.cnt = 0; }

constexpr int SYM_TRUNCATED = -1, SYM_NONE = -2;

// One symbol of a canonical code, bit by bit: the code of length len is `code`, the first code of that length is `first`.
MXY_HD int decode_sym(BitReader& b, const uint16_t* count, const uint16_t* sym) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        uint32_t bit;
        if (!br_take(b, 1, bit)) return SYM_TRUNCATED;
        code |= (int)bit;
        const int c = count[len];
        if (code - c < first) return sym[index + (code - first)];
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    return SYM_NONE;   // an incomplete code, and these bits are none of its codes
}
MXY_HD int decode_lit(BitReader& b, const Tables& t) {
    br_fill(b);
    const uint32_t e = t.fast[(uint32_t)b.buf & (FAST_SIZE - 1u)];
    const uint32_t bits = e & 15u;
    if (e && bits <= b.cnt) { b.buf >>= bits; b.cnt -= bits; return (int)(e >> 4); }
    return decode_sym(b, t.len_count, t.len_sym);
}

enum CodeKind { CODE_LENGTHS = 0, CODE_LITLEN = 1, CODE_DIST = 2 };

// lens[0, n) -> count[16] and sym[n] (and t.fast for CODE_LITLEN). GZ_OK or GZ_BAD_CODES.
MXY_HD int32_t build_code(Tables& t, const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* sym, CodeKind kind) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) count[lens[i] & 15u]++;
    int max = 15;
    while (max > 0 && count[max] == 0) --max;
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return GZ_BAD_CODES;   // over-subscribed
    }
    if (max == 0) {                          // no code at all: every symbol read through it fails; a code-length code cannot be empty
        if (kind == CODE_LENGTHS) return GZ_BAD_CODES;
    } else if (left > 0 && (kind == CODE_LENGTHS || max != 1)) return GZ_BAD_CODES;   // incomplete
    t.offs[1] = 0; t.next[1] = 0;
    for (int l = 1; l < 15; ++l) {
        t.offs[l + 1] = (uint16_t)(t.offs[l] + count[l]);
        t.next[l + 1] = (uint16_t)((t.next[l] + count[l]) << 1);
    }
    if (kind == CODE_LITLEN) for (uint32_t i = 0; i < FAST_SIZE; ++i) t.fast[i] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i] & 15u;
        if (!l) continue;
        sym[t.offs[l]++] = (uint16_t)i;
        const uint32_t code = t.next[l]++;
        if (kind != CODE_LITLEN || l > FAST_BITS) continue;
        uint32_t rev = 0;
        for (uint32_t k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1u - k);
        for (uint32_t e = rev; e < FAST_SIZE; e += 1u << l) t.fast[e] = (uint16_t)(i << 4 | l);
    }
    return GZ_OK;
}

MXY_HD int32_t build_fixed(Tables& t) {
    for (uint32_t i = 0; i < 288u; ++i) t.lens[i] = (uint8_t)(i < 144u ? 8 : i < 256u ? 9 : i < 280u ? 7 : 8);
    for (uint32_t i = 288u; i < 320u; ++i) t.lens[i] = 5;   // 32 distance codes: 30 and 31 decode, and are refused as symbols
    const int32_t e = build_code(t, t.lens, 288, t.len_count, t.len_sym, CODE_LITLEN);
    return e ? e : build_code(t, t.lens + 288, 32, t.dist_count, t.dist_sym, CODE_DIST);
}

// The header of a dynamic block. GZ_OK, GZ_TRUNCATED or GZ_BAD_CODES.
MXY_HD int32_t read_dynamic(BitReader& b, Tables& t) {
    uint32_t hlit, hdist, hclen, v;
    if (!br_take(b, 5, hlit) || !br_take(b, 5, hdist) || !br_take(b, 4, hclen)) return GZ_TRUNCATED;
    hlit += 257u; hdist += 1u; hclen += 4u;
    if (hlit > 286u || hdist > 30u) return GZ_BAD_CODES;
    // the order of the code-length code's lengths, five bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    for (uint32_t i = 0; i < 19u; ++i) t.lens[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        if (!br_take(b, 3, v)) return GZ_TRUNCATED;
        const uint32_t at = (uint32_t)((i < 12u ? order_lo >> (5u * i) : order_hi >> (5u * (i - 12u))) & 31u);
        t.lens[at] = (uint8_t)v;
    }
    if (build_code(t, t.lens, 19, t.dist_count, t.dist_sym, CODE_LENGTHS)) return GZ_BAD_CODES;
    const uint32_t total = hlit + hdist;
    for (uint32_t idx = 0; idx < total;) {
        const int s = decode_sym(b, t.dist_count, t.dist_sym);
        if (s < 0) return s == SYM_TRUNCATED ? GZ_TRUNCATED : GZ_BAD_CODES;
        if (s < 16) { t.lens[idx++] = (uint8_t)s; continue; }
        uint32_t prev = 0, rep;
        if (s == 16) {
            if (idx == 0) return GZ_BAD_CODES;   // nothing to repeat
            prev = t.lens[idx - 1];
            if (!br_take(b, 2, v)) return GZ_TRUNCATED;
            rep = 3u + v;
        } else if (s == 17) {
            if (!br_take(b, 3, v)) return GZ_TRUNCATED;
            rep = 3u + v;
        } else {
            if (!br_take(b, 7, v)) return GZ_TRUNCATED;
            rep = 11u + v;
        }
        if (idx + rep > total) return GZ_BAD_CODES;   // a repeat may cross from the literal/length lengths into the distance lengths, not past both
        for (uint32_t k = 0; k < rep; ++k) t.lens[idx++] = (uint8_t)prev;
    }
    if (t.lens[256] == 0) return GZ_BAD_CODES;   // no end of block
    // the code-length code in dist_count / dist_sym is done with: the distance code takes its place
    if (build_code(t, t.lens, hlit, t.len_count, t.len_sym, CODE_LITLEN)) return GZ_BAD_CODES;
    return build_code(t, t.lens + hlit, hdist, t.dist_count, t.dist_sym, CODE_DIST);
}

// A token: `pos` is the first output byte it writes (relative to the member). v: bit 31 clear = literal, the byte in bits 0..7; bit 31
// set = match, length (3..258) in bits 0..8 and distance (1..32768) in bits 9..24.
struct Token { uint32_t pos, v; };
constexpr uint32_t TOKEN_MATCH = 0x80000000u;
MXY_HD bool token_is_match(const Token& t) { return (t.v & TOKEN_MATCH) != 0; }
MXY_HD uint32_t token_len(const Token& t) { return t.v & 511u; }
MXY_HD uint32_t token_dist(const Token& t) { return (t.v >> 9) & 0xFFFFu; }
// byte i of a match at `pos` is a copy of this byte; a distance below the length repeats the last `dist` bytes
MXY_HD uint32_t match_src(uint32_t pos, uint32_t dist, uint32_t i) { return pos - dist + (i < dist ? i : i % dist); }

struct Decoder {
    BitReader br;
    uint32_t produced, cap;   // bytes handed out as tokens so far; the member's capacity
    int32_t status;           // GZ_OK while the stream is sound
    bool in_block, final, done;   // inside a Huffman block; the block in hand is the last; the last block has ended
};
MXY_HD void decoder_init(Decoder& d, const uint8_t* in, uint32_t in_len, uint32_t cap) {
    d.br.in = in; d.br.pos = 0; d.br.end = in_len; d.br.buf = 0; d.br.cnt = 0;
    d.produced = 0; d.cap = cap; d.status = GZ_OK;
    d.in_block = false; d.final = false; d.done = false;
}

// What one call of decode_batch hands out: q[0, n) in stream order, then (stored_len != 0) stored_len bytes from in[stored_src ..) to
// stored_pos. The executor writes the literals, then the matches one after another, then the stored run.
struct Batch { uint32_t n, stored_src, stored_len, stored_pos; };

// Decodes until the queue is full, a stored run is due, the stream ends (d.done) or an error (d.status).
MXY_HD void decode_batch(Decoder& d, Tables& t, Token* q, uint32_t max_q, Batch& out) {
    BitReader& b = d.br;
    out.n = 0; out.stored_src = 0; out.stored_len = 0; out.stored_pos = 0;
    uint32_t v;
    while (out.n < max_q && !d.done && d.status == GZ_OK) {
        if (!d.in_block) {
            if (d.final) { d.done = true; break; }
            uint32_t type;
            if (!br_take(b, 1, v) || !br_take(b, 2, type)) { d.status = GZ_TRUNCATED; break; }
            d.final = v != 0;
            if (type == 0) {
                uint32_t len, nlen;
                (void)br_align(b);
                if (!br_take(b, 16, len) || !br_take(b, 16, nlen)) { d.status = GZ_TRUNCATED; break; }
                if ((len ^ 0xFFFFu) != nlen) { d.status = GZ_BAD_BLOCK; break; }
                const uint32_t at = br_align(b);
                if (len > b.end - at) { d.status = GZ_TRUNCATED; break; }
                if (len > d.cap - d.produced) { d.status = GZ_OVERFLOW; break; }
                br_seek(b, at + len);
                if (len) {
                    out.stored_src = at; out.stored_len = len; out.stored_pos = d.produced;
                    d.produced += len;
                    break;   // what follows may copy from these bytes: they are written first
                }
            } else if (type == 1) {
                d.status = build_fixed(t);
                d.in_block = true;
            } else if (type == 2) {
                d.status = read_dynamic(b, t);
                d.in_block = true;
            } else d.status = GZ_BAD_BLOCK;
            continue;
        }
        const int s = decode_lit(b, t);
        if (s < 0) { d.status = s == SYM_TRUNCATED ? GZ_TRUNCATED : GZ_BAD_SYMBOL; break; }
        if (s < 256) {
            if (d.produced >= d.cap) { d.status = GZ_OVERFLOW; break; }
            q[out.n].pos = d.produced++; q[out.n].v = (uint32_t)s; ++out.n;
            continue;
        }
        if (s == 256) { d.in_block = false; continue; }
        if (s >= 286) { d.status = GZ_BAD_SYMBOL; break; }
        // lengths 3..258 from symbols 257..285, distances 1..32768 from symbols 0..29: base and extra bits follow from the symbol
        const uint32_t ls = (uint32_t)s - 257u;
        uint32_t len = 3u + ls;
        if (ls == 28u) len = 258u;
        else if (ls >= 8u) {
            const uint32_t eb = (ls >> 2) - 1u;
            if (!br_take(b, eb, v)) { d.status = GZ_TRUNCATED; break; }
            len = 3u + ((4u + (ls & 3u)) << eb) + v;
        }
        const int ds = decode_sym(b, t.dist_count, t.dist_sym);
        if (ds < 0) { d.status = ds == SYM_TRUNCATED ? GZ_TRUNCATED : GZ_BAD_SYMBOL; break; }
        if (ds >= 30) { d.status = GZ_BAD_SYMBOL; break; }
        uint32_t dist = 1u + (uint32_t)ds;
        if (ds >= 4) {
            const uint32_t eb = ((uint32_t)ds >> 1) - 1u;
            if (!br_take(b, eb, v)) { d.status = GZ_TRUNCATED; break; }
            dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + v;
        }
        if (dist > d.produced) { d.status = GZ_BAD_DISTANCE; break; }
        if (len > d.cap - d.produced) { d.status = GZ_OVERFLOW; break; }
        q[out.n].pos = d.produced; q[out.n].v = TOKEN_MATCH | len | dist << 9; ++out.n;
        d.produced += len;
    }
}

// Behind a stream that ended (d.done): the 8-byte trailer follows the last block's last byte. `crc` is the CRC-32 of the output.
MXY_HD int32_t check_trailer(Decoder& d, uint32_t crc) {
    const uint32_t at = br_align(d.br);
    const BitReader& b = d.br;
    if (b.end - at < 8u) return GZ_TRUNCATED;
    const uint8_t* p = b.in + at;
    const uint32_t want_crc = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    const uint32_t isize = p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
    if (d.produced != d.cap || isize != d.produced) return GZ_SIZE_MISMATCH;
    if (want_crc != crc) return GZ_CRC_MISMATCH;
    return b.end - at == 8u ? GZ_OK : GZ_TRAILING_DATA;
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320) in pieces: a lane takes crc_bytes over its chunk, multiplies it by x^(8 * bytes behind
// the chunk) mod the polynomial, and the xor of all lanes' products is the CRC of the whole (the CRC of the empty string is 0).
constexpr uint32_t CRC_POLY = 0xEDB88320u;
MXY_HD uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? CRC_POLY ^ (c >> 1) : c >> 1;
    return c;
}
MXY_HD uint32_t crc_bytes(const uint32_t* table, const uint8_t* p, uint32_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}
// a * b mod the polynomial, bit 31 = x^0: 32 shift-and-xor steps
MXY_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 31; k >= 0; --k) {
        if (a >> k & 1u) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 * nbytes): square and multiply over the 35 bits of the exponent
MXY_HD uint32_t crc_xpow8(uint32_t nbytes) {
    uint64_t e = (uint64_t)nbytes * 8u;
    uint32_t r = 0x80000000u, sq = 0x40000000u;   // x^0, x^1
    for (int k = 0; k < 36 && e; ++k, e >>= 1) {
        if (e & 1u) r = crc_mul(sq, r);
        sq = crc_mul(sq, sq);
    }
    return r;
}
// chunk of lane `lane` of `lanes` over n bytes: [begin, begin + len)
MXY_HD void crc_chunk(uint32_t n, uint32_t lane, uint32_t lanes, uint32_t& begin, uint32_t& len) {
    const uint32_t per = (n + lanes - 1u) / lanes;
    begin = lane * per < n ? lane * per : n;
    len = n - begin < per ? n - begin : per;
}
MXY_HD uint32_t crc_lane_part(const uint32_t* table, const uint8_t* out, uint32_t n, uint32_t lane, uint32_t lanes) {
    uint32_t begin, len;
    crc_chunk(n, lane, lanes, begin, len);
    if (!len) return 0;
    return crc_mul(crc_bytes(table, out + begin, len), crc_xpow8(n - begin - len));
}

// ------------------------------------------------------------------------------------------------ pieces of one stream
// One large member is cut into pieces of piece_bytes compressed bytes (inflate_pieces.hip). Piece 0 starts at bit 0 of the body; every
// other piece starts at the first bit position inside it where a dynamic block header parses (piece_probe), if there is one. Every piece
// is decoded from its start with no knowledge of the 32 KiB in front of it: a back-reference that reaches in front of the piece's first
// byte becomes a MARKER symbol (256 + k: byte k of those 32 KiB). A piece stops at the first block end that is the start of a later
// piece; the pieces reached from piece 0 by following these landings are LIVE, and because every live piece starts at the bit where the
// one in front ended, a chain that reaches the end of the final block is the sequential parse of the stream. A false start is never live.
//
// Loop bounds: the probe reads at most 74 bits in front of read_dynamic; a piece decoder consumes at least one input bit per token or
// block header (the turn bound of its callers is 8 * body_len + 2, as for decode_batch), ends at the member's end or capacity, and —
// any piece but piece 0 — after it has passed GZ_PIECE_MAX_SKIP candidate starts without landing on one.

// Bit positions are relative to the member's body and 64-bit: a body of 4 GiB has 2^35 of them.
MXY_HD uint64_t br_bit_pos(const BitReader& b) { return (uint64_t)b.pos * 8u - b.cnt; }
MXY_HD void br_seek_bit(BitReader& b, uint64_t bit) {
    const uint64_t byte = bit >> 3;
    br_seek(b, byte < b.end ? (uint32_t)byte : b.end);
    const uint32_t drop = (uint32_t)bit & 7u;
    if (!drop || byte >= b.end) return;
    br_fill(b);   // at least one byte: cnt >= 8 > drop
    b.buf >>= drop; b.cnt -= drop;
}

// n <= 24 bits at bit position `bit` of in[0, end), low bit first; false: the input ends first
MXY_HD bool peek_bits(const uint8_t* in, uint32_t end, uint64_t bit, uint32_t n, uint32_t& v) {
    if (bit + n > (uint64_t)end * 8u) return false;
    const uint32_t at = (uint32_t)(bit >> 3), sh = (uint32_t)bit & 7u;
    uint32_t w = 0;
    for (uint32_t k = 0; k < 4u && at + k < end; ++k) w |= (uint32_t)in[at + k] << (8u * k);
    v = (w >> sh) & ((1u << n) - 1u);
    return true;
}

// The cheap test in front of the probe: any BFINAL, BTYPE = 2, HLIT <= 29, HDIST <= 29 and a code-length code whose Kraft sum is exactly
// 1 (build_code refuses every other one for CODE_LENGTHS). 17 + 3 * (HCLEN + 4) <= 74 bits, nothing stored.
MXY_HD bool piece_probe_cheap(const uint8_t* in, uint32_t end, uint64_t bit) {
    uint32_t h;
    if (!peek_bits(in, end, bit, 17, h)) return false;
    if (((h >> 1) & 3u) != 2u || ((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = ((h >> 13) & 15u) + 4u;
    uint32_t kraft = 0;   // in units of 2^-7
    for (uint32_t i = 0; i < hclen; i += 8u) {   // <= 3 turns of <= 8 lengths
        const uint32_t n = hclen - i < 8u ? hclen - i : 8u;
        uint32_t w;
        if (!peek_bits(in, end, bit + 17u + 3u * i, 3u * n, w)) return false;
        for (uint32_t k = 0; k < n; ++k) { const uint32_t l = (w >> (3u * k)) & 7u; if (l) kraft += 128u >> l; }
    }
    return kraft == 128u;
}
// A block start at `bit`: the cheap test, then a dynamic header that read_dynamic accepts. Stored and fixed blocks have no findable
// start: the piece in front decodes them. t is scratch.
MXY_HD bool piece_probe(const uint8_t* in, uint32_t end, uint64_t bit, Tables& t) {
    if (!piece_probe_cheap(in, end, bit)) return false;
    BitReader b;
    b.in = in; b.end = end;
    br_seek_bit(b, bit + 3u);
    return read_dynamic(b, t) == GZ_OK;
}

// A piece that is no piece 0 gives up after it has passed this many candidate starts without landing on one. A true start lands on the
// next true start; between two true starts lie only false candidates, which the probe rarely lets through (none in the 1 MB of
// compressed log text of the test vectors; the dead candidates of the false-start vector are genuine headers inside a stored
// payload). 8 passed candidates therefore mean a run of 8 pieces' worth of stored or fixed blocks or of false starts — a false start that
// happens to decode on is cut off after about 8 pieces of input in place of the member's rest, and a true start that gives up only
// makes its member take the one-wave path, which is always right.
constexpr uint32_t GZ_PIECE_MAX_SKIP = 8;
constexpr uint32_t GZ_PIECE_WINDOW = 32768;
constexpr uint32_t GZ_PIECE_QUEUE = 64;   // tokens per call of piece_decode_batch, for the kernels and the CPU driver alike
constexpr uint64_t GZ_PIECE_NO_START = ~0ull;
constexpr uint32_t GZ_PIECE_END = 0xFFFFFFFFu, GZ_PIECE_NONE = 0xFFFFFFFEu;   // landed on the end of the final block; not landed
constexpr int32_t GZ_PIECE_NO_LANDING = 11;   // internal to the piece table, never a member's status

// A symbol of the scratch: 0..255 a byte, 256 + k byte k of the GZ_PIECE_WINDOW bytes in front of the piece's first byte.
constexpr uint32_t GZ_SYM_MARKER = 256;
// Symbol i of a match at piece position `pos`: the index of the symbol it copies, or (negative) -1 - k for window byte k.
MXY_HD int32_t piece_match_src(uint32_t pos, uint32_t dist, uint32_t i) {
    const int64_t src = (int64_t)pos - (int64_t)dist + (int64_t)(i < dist ? i : i % dist);
    return src >= 0 ? (int32_t)src : (int32_t)(-1 - ((int64_t)GZ_PIECE_WINDOW + src));
}

// decode_batch for a piece: it starts at start_bit with produced = 0, allows a distance up to `window` bytes in front of the piece
// (0 for piece 0, which keeps the rule of decode_batch), and stops at a block end that is a candidate start behind it.
// starts[0, n_pieces) are the pieces' start bits, sorted by construction (piece i's lies inside piece i), GZ_PIECE_NO_START for none.
struct PieceDecoder {
    Decoder d;
    const uint64_t* starts;
    uint32_t n_pieces, self, nc;   // nc: the first piece behind `self` whose start has not been passed
    uint32_t window, skipped, landed;
    uint64_t end_bit;
};
MXY_HD void piece_decoder_init(PieceDecoder& p, const uint8_t* in, uint32_t in_len, uint32_t cap, const uint64_t* starts, uint32_t n_pieces, uint32_t self, uint64_t start_bit) {
    decoder_init(p.d, in, in_len, cap);
    br_seek_bit(p.d.br, start_bit);
    p.starts = starts; p.n_pieces = n_pieces; p.self = self; p.nc = self + 1u;
    p.window = self ? GZ_PIECE_WINDOW : 0u;
    p.skipped = 0; p.landed = GZ_PIECE_NONE; p.end_bit = start_bit;
}
// Counts the candidates in front of bit `at`: no block end can land on them any more. Every turn advances nc.
MXY_HD void piece_pass_candidates(PieceDecoder& p, uint64_t at) {
    while (p.nc < p.n_pieces && (p.starts[p.nc] == GZ_PIECE_NO_START || p.starts[p.nc] < at)) {
        if (p.starts[p.nc] != GZ_PIECE_NO_START) ++p.skipped;
        ++p.nc;
    }
    if (p.self && p.skipped >= GZ_PIECE_MAX_SKIP) p.d.status = GZ_PIECE_NO_LANDING;
}
// At a block end (the final block's aside): lands on a candidate at this bit, or counts the candidates passed.
MXY_HD void piece_block_end(PieceDecoder& p) {
    const uint64_t at = br_bit_pos(p.d.br);
    piece_pass_candidates(p, at);
    if (p.d.status == GZ_OK && p.nc < p.n_pieces && p.starts[p.nc] == at) { p.landed = p.nc; p.d.done = true; }
}
// Decodes until the queue is full, a stored run is due, the piece has landed or the stream has ended (d.done, p.landed), or an error.
// A match token's `pos` is relative to the piece; its distance may exceed pos by up to p.window.
MXY_HD void piece_decode_batch(PieceDecoder& p, Tables& t, Token* q, uint32_t max_q, Batch& out) {
    Decoder& d = p.d;
    BitReader& b = d.br;
    out.n = 0; out.stored_src = 0; out.stored_len = 0; out.stored_pos = 0;
    uint32_t v;
    // once per call, inside a block too: a false start whose block never ends gives up max_q tokens behind the last candidate it may
    // pass, not at the member's capacity. Where a piece gives up therefore depends on max_q, which is GZ_PIECE_QUEUE for every caller.
    if (!d.done && d.status == GZ_OK) piece_pass_candidates(p, br_bit_pos(b));
    while (out.n < max_q && !d.done && d.status == GZ_OK) {
        if (!d.in_block) {
            uint32_t type;
            if (!br_take(b, 1, v) || !br_take(b, 2, type)) { d.status = GZ_TRUNCATED; break; }
            d.final = v != 0;
            if (type == 0) {
                uint32_t len, nlen;
                (void)br_align(b);
                if (!br_take(b, 16, len) || !br_take(b, 16, nlen)) { d.status = GZ_TRUNCATED; break; }
                if ((len ^ 0xFFFFu) != nlen) { d.status = GZ_BAD_BLOCK; break; }
                const uint32_t at = br_align(b);
                if (len > b.end - at) { d.status = GZ_TRUNCATED; break; }
                if (len > d.cap - d.produced) { d.status = GZ_OVERFLOW; break; }
                br_seek(b, at + len);
                out.stored_src = at; out.stored_len = len; out.stored_pos = d.produced;
                d.produced += len;
                if (d.final) { d.done = true; p.landed = GZ_PIECE_END; } else piece_block_end(p);
                if (len) break;   // what follows may copy from these bytes: they are written first
            } else if (type == 1) {
                d.status = build_fixed(t);
                d.in_block = true;
            } else if (type == 2) {
                d.status = read_dynamic(b, t);
                d.in_block = true;
            } else d.status = GZ_BAD_BLOCK;
            continue;
        }
        const int s = decode_lit(b, t);
        if (s < 0) { d.status = s == SYM_TRUNCATED ? GZ_TRUNCATED : GZ_BAD_SYMBOL; break; }
        if (s < 256) {
            if (d.produced >= d.cap) { d.status = GZ_OVERFLOW; break; }
            q[out.n].pos = d.produced++; q[out.n].v = (uint32_t)s; ++out.n;
            continue;
        }
        if (s == 256) {
            d.in_block = false;
            if (d.final) { d.done = true; p.landed = GZ_PIECE_END; } else piece_block_end(p);
            continue;
        }
        if (s >= 286) { d.status = GZ_BAD_SYMBOL; break; }
        const uint32_t ls = (uint32_t)s - 257u;
        uint32_t len = 3u + ls;
        if (ls == 28u) len = 258u;
        else if (ls >= 8u) {
            const uint32_t eb = (ls >> 2) - 1u;
            if (!br_take(b, eb, v)) { d.status = GZ_TRUNCATED; break; }
            len = 3u + ((4u + (ls & 3u)) << eb) + v;
        }
        const int ds = decode_sym(b, t.dist_count, t.dist_sym);
        if (ds < 0) { d.status = ds == SYM_TRUNCATED ? GZ_TRUNCATED : GZ_BAD_SYMBOL; break; }
        if (ds >= 30) { d.status = GZ_BAD_SYMBOL; break; }
        uint32_t dist = 1u + (uint32_t)ds;
        if (ds >= 4) {
            const uint32_t eb = ((uint32_t)ds >> 1) - 1u;
            if (!br_take(b, eb, v)) { d.status = GZ_TRUNCATED; break; }
            dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + v;
        }
        if (dist > d.produced && dist - d.produced > p.window) { d.status = GZ_BAD_DISTANCE; break; }
        if (len > d.cap - d.produced) { d.status = GZ_OVERFLOW; break; }
        q[out.n].pos = d.produced; q[out.n].v = TOKEN_MATCH | len | dist << 9; ++out.n;
        d.produced += len;
    }
    if (d.done || d.status != GZ_OK) p.end_bit = br_bit_pos(b);
}

// One piece as the passes hand it on. Filled by the find (start_bit, FLAG_START), the count (end_bit, next, produced, status), the chain
// (out_pos, FLAG_LIVE) and the verdict (FLAG_HANDED); member and sym_base come from the host. The first 32 bytes are matchy_gz_piece_t.
struct Piece {
    uint64_t start_bit, end_bit;
    uint32_t member, produced, out_pos, flags;
    uint32_t next, crc, sym_base;   // sym_base: where the member's symbols begin in the scratch
    int32_t status;
};
static_assert(sizeof(Piece) == 48, "matchy_gz_piece_t and the passes' own four words");
constexpr uint32_t PIECE_HAS_START = 1, PIECE_LIVE = 2, PIECE_HANDED = 4;

// The find for piece i of a member whose body has body_len bytes: the first candidate in [i * piece_bytes * 8, (i + 1) * piece_bytes * 8)
// and in front of the body's end. At most 8 * piece_bytes offsets. (The kernel tries 64 per turn; the result is the same.)
MXY_HD uint64_t piece_find(const uint8_t* in, uint32_t body_len, uint32_t piece_bytes, uint32_t i, Tables& t) {
    if (i == 0) return 0;
    const uint64_t lo = (uint64_t)i * piece_bytes * 8u, total = (uint64_t)body_len * 8u;
    const uint64_t hi = lo + (uint64_t)piece_bytes * 8u < total ? lo + (uint64_t)piece_bytes * 8u : total;
    for (uint64_t bit = lo; bit < hi; ++bit) if (piece_probe(in, body_len, bit, t)) return bit;
    return GZ_PIECE_NO_START;
}

// The chain of one member over pieces[0, n): walks from piece 0 along `next` (strictly increasing: at most n turns), sets out_pos and
// PIECE_LIVE, and returns whether the chain is complete: it reaches the end of the final block through pieces that are all OK, their
// bytes sum to `cap`, and exactly the 8 bytes of a trailer whose ISIZE is `cap` follow the last block's last byte. (The CRC is the
// resolve pass's.)
MXY_HD bool piece_chain(Piece* pieces, uint32_t n, const uint8_t* in, uint32_t body_len, uint32_t cap) {
    uint64_t sum = 0;
    uint32_t i = 0;
    for (uint32_t turn = 0; turn < n; ++turn) {
        Piece& p = pieces[i];
        if (!(p.flags & PIECE_HAS_START) || p.status != GZ_OK || sum + p.produced > cap) return false;
        p.out_pos = (uint32_t)sum; p.flags |= PIECE_LIVE;
        sum += p.produced;
        if (p.next == GZ_PIECE_END) {
            const uint64_t at = (p.end_bit + 7u) >> 3;
            if (sum != cap || at > body_len || body_len - at != 8u) return false;
            const uint8_t* t = in + at + 4;
            return ((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24) == cap;
        }
        if (p.next <= i || p.next >= n) return false;
        i = p.next;
    }
    return false;
}

// A symbol to its byte: text[0, cap) is the member's text, pos the symbol's position in it, piece_pos its piece's out_pos. False: a
// marker that points in front of the member's first byte (the sequential path calls it BAD_DISTANCE).
MXY_HD bool piece_resolve_sym(uint32_t sym, const uint8_t* text, uint32_t piece_pos, uint8_t& byte) {
    if (sym < GZ_SYM_MARKER) { byte = (uint8_t)sym; return true; }
    const uint32_t k = sym - GZ_SYM_MARKER;
    if (k >= GZ_PIECE_WINDOW || piece_pos + k < GZ_PIECE_WINDOW) return false;
    byte = text[piece_pos - GZ_PIECE_WINDOW + k];
    return true;
}


// ------------------------------------------------------------------------------------------------ windows of one stream
// One DEFLATE stream that is larger than a batch goes through the passes above as a chain of STREAM WINDOWS (inflate_pieces.hip "stream
// windows", gz_stream.h for the host's side). A window is a run in[0, in_len) of the stream's compressed bytes whose first block starts at
// bit `bit` (0..7) of in[0]; the text in front of it has text_bytes bytes, CRC-32 `crc` and the last history_len = min(text_bytes, 32768)
// of them are history[0, history_len). The window is cut into pieces like a split member, with three differences: piece 0 starts at
// `bit`; piece 0 allows distances up to history_len beyond its own bytes (they become markers, like every later piece's); and the chain
// is OPEN: it ends in front of the first piece that cannot be taken, and where it ends is where the next window begins. Every live piece
// starts at the bit where the one in front ended and piece 0 starts at a true block start, so the end of every live piece is a true
// block end of the stream. Piece 0 still never gives up on passed candidates (piece_pass_candidates tests p.self).
struct StreamState {
    uint64_t text_bytes;
    uint32_t crc, bit, history_len;
    uint8_t history[GZ_PIECE_WINDOW];
};
static_assert(sizeof(StreamState) == 24 + GZ_PIECE_WINDOW, "matchy_gz_stream_state_t");
// a state a caller may hand in
MXY_HD bool stream_state_valid(uint64_t text_bytes, uint32_t bit, uint32_t history_len) {
    return bit <= 7u && history_len <= GZ_PIECE_WINDOW && history_len <= text_bytes;
}

// Status of a window, bit-identical to MATCHY_STREAM_* (include/matchy_amd.h); NO_LINE_END has the value of GZ_WINDOW_NO_LINE_END and is
// the line tail's.
enum : int32_t { STREAM_OK = 0, STREAM_NO_LINE_END = 1, STREAM_NO_PROGRESS = 2, STREAM_FAILED = 3 };

// piece_find for a window: piece 0 starts at the state's bit
MXY_HD uint64_t stream_piece_find(const uint8_t* in, uint32_t in_len, uint32_t piece_bytes, uint32_t i, uint32_t bit, Tables& t) {
    return i == 0 ? (uint64_t)bit : piece_find(in, in_len, piece_bytes, i, t);
}
// piece_decoder_init for a window: piece 0 may reach history_len bytes in front of itself. A distance beyond produced + history_len
// stays GZ_BAD_DISTANCE (the preset-dictionary case of the first window, whose history is empty).
MXY_HD void stream_piece_decoder_init(PieceDecoder& p, const uint8_t* in, uint32_t in_len, uint32_t cap, const uint64_t* starts, uint32_t n_pieces, uint32_t self,
                                      uint64_t start_bit, uint32_t history_len) {
    piece_decoder_init(p, in, in_len, cap, starts, n_pieces, self, start_bit);
    if (self == 0) p.window = history_len < GZ_PIECE_WINDOW ? history_len : GZ_PIECE_WINDOW;
}

// What the open chain of a window found. n_live == 0: no progress, or (failed != GZ_OK) piece 0, which starts at a true block start,
// met an error of the stream itself; the end of the input and the capacity are no such errors: a later window may hold more.
struct StreamChain {
    uint64_t consumed_bits;   // the end bit of the last live piece, relative to in[0]
    uint32_t n_live, text_len, last;   // last: the last live piece
    int32_t failed;
    bool ended;               // the last live piece landed on the end of the final block
};
// The open chain over pieces[0, n): walks from piece 0 along `next` (strictly increasing: at most n turns), sets out_pos and PIECE_LIVE, and
// stops, without failing, in front of the first piece that has no start, is not OK, has not landed or would take the sum above `cap`. A
// piece that lands on the end of the final block is live only with file_end (the window's bytes reach the file's end): the trailer
// behind it belongs to the window that can see all of it.
MXY_HD StreamChain stream_chain(Piece* pieces, uint32_t n, uint32_t cap, bool file_end) {
    StreamChain c;
    c.consumed_bits = 0; c.n_live = 0; c.text_len = 0; c.last = 0; c.failed = GZ_OK; c.ended = false;
    uint64_t sum = 0;
    uint32_t i = 0;
    for (uint32_t turn = 0; turn < n; ++turn) {
        Piece& p = pieces[i];
        if (!(p.flags & PIECE_HAS_START) || p.status != GZ_OK || sum + p.produced > cap) break;
        const bool end = p.next == GZ_PIECE_END;
        if (end ? !file_end : (p.next <= i || p.next >= n)) break;
        p.out_pos = (uint32_t)sum; p.flags |= PIECE_LIVE;
        sum += p.produced;
        c.consumed_bits = p.end_bit; c.last = i; ++c.n_live;
        if (end) { c.ended = true; break; }
        i = p.next;
    }
    c.text_len = (uint32_t)sum;
    if (c.n_live == 0 && n != 0 && (pieces[0].flags & PIECE_HAS_START)) {
        const int32_t st = pieces[0].status;
        if (st == GZ_BAD_BLOCK || st == GZ_BAD_CODES || st == GZ_BAD_SYMBOL || st == GZ_BAD_DISTANCE) c.failed = st;
    }
    return c;
}

// piece_resolve_sym for a window: a marker that points in front of the window's first text byte reads the history, one that points in
// front of the history fails (GZ_BAD_DISTANCE). text is the window's text, piece_pos the piece's out_pos in it.
MXY_HD bool stream_resolve_sym(uint32_t sym, const uint8_t* text, uint32_t piece_pos, const uint8_t* history, uint32_t history_len, uint8_t& byte) {
    if (sym < GZ_SYM_MARKER) { byte = (uint8_t)sym; return true; }
    const uint32_t k = sym - GZ_SYM_MARKER;
    if (k >= GZ_PIECE_WINDOW) return false;
    const int64_t at = (int64_t)piece_pos + (int64_t)k - (int64_t)GZ_PIECE_WINDOW;
    if (at >= 0) { byte = text[at]; return true; }
    if (-at > (int64_t)history_len || history_len > GZ_PIECE_WINDOW) return false;
    byte = history[(int64_t)history_len + at];
    return true;
}

// A piece's CRC times x^(8 * bytes behind it in the window): text_len, not the capacity, is the window's end.
MXY_HD uint32_t stream_piece_crc(uint32_t piece_crc, uint32_t text_len, uint32_t out_pos, uint32_t produced) {
    return crc_mul(piece_crc, crc_xpow8(text_len - out_pos - produced));
}
// CRC-32 of (text in front ‖ window text) from the two CRCs
MXY_HD uint32_t stream_crc_combine(uint32_t crc_before, uint32_t window_crc, uint32_t text_len) { return crc_mul(crc_before, crc_xpow8(text_len)) ^ window_crc; }
// ISIZE is the stream's length modulo 2^32
MXY_HD uint32_t stream_isize(uint64_t text_bytes, uint32_t text_len) { return (uint32_t)((text_bytes + text_len) & 0xFFFFFFFFull); }

// The stream ended in this window, whose bytes reach the file's end: exactly the 8 bytes of the trailer follow the last block's last
// byte, ISIZE is the whole text's length and the CRC the whole text's. The order is check_trailer's: TRUNCATED, SIZE_MISMATCH,
// CRC_MISMATCH, TRAILING_DATA.
MXY_HD int32_t stream_end_check(const uint8_t* in, uint32_t in_len, uint64_t end_bit, uint64_t text_bytes, uint32_t text_len, uint32_t crc) {
    const uint64_t at = (end_bit + 7u) >> 3;
    if (at > in_len || in_len - at < 8u) return GZ_TRUNCATED;
    const uint8_t* p = in + at;
    const uint32_t want_crc = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    const uint32_t isize = p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
    if (isize != stream_isize(text_bytes, text_len)) return GZ_SIZE_MISMATCH;
    if (want_crc != crc) return GZ_CRC_MISMATCH;
    return in_len - at == 8u ? GZ_OK : GZ_TRAILING_DATA;
}

// The history behind a window: the last min(32768, history_len + text_len) bytes of history ‖ text. Byte j of it. (The kernel copies
// one byte per lane and turn; out and history do not overlap.)
MXY_HD uint32_t stream_history_len(uint32_t history_len, uint32_t text_len) {
    const uint64_t all = (uint64_t)history_len + text_len;
    return all < GZ_PIECE_WINDOW ? (uint32_t)all : GZ_PIECE_WINDOW;
}
MXY_HD uint8_t stream_history_byte(const uint8_t* history, uint32_t history_len, const uint8_t* text, uint32_t text_len, uint32_t new_len, uint32_t j) {
    const uint64_t at = (uint64_t)history_len + text_len - new_len + j;   // position in history ‖ text
    return at < history_len ? history[at] : text[at - history_len];
}

}  // namespace gz
}  // namespace mxy
