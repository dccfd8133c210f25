// CPU: the piece rules of inflate_core.h (pieces of one stream, matchy_amd/csrc/inflate_pieces.hip) driven sequentially through all
// passes, the way the kernels drive them: find, count (dry), chain, symbols (into 16-bit symbols), windows (the last 32 KiB of every
// live piece, in chain order), resolve (the rest, and the CRC-32 as one part per piece), verdict, and the handover of a member whose
// chain is not complete to the sequential decoder. Built with -fsanitize=address,undefined (tests/test_gz_pieces_host.py): the member
// lives in a heap block of exactly its length, symbols and text in blocks of exactly the capacity, so a load behind the member's end or
// a store outside a piece's own range stops the run.
//
//   test_gz_pieces CASES OUT PIECE_BYTES   CASES: u32 n, then per case u32 len, u32 out_len, bytes (tests/gz_cases.py)
//                                          OUT:   per case i32 status, u32 n, n bytes (the text of an OK member), u32 n_pieces,
//                                                 n_pieces * 32 bytes (matchy_gz_piece_t)
// stdout: one line per case and one per piece.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gz_plan.h"
#include "inflate_core.h"

using namespace mxy;

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(3); }

static int32_t inflate_member(const uint8_t* body, uint32_t body_len, uint8_t* out, uint32_t cap, gz::Tables& tab, const uint32_t* crc_tab) {
    gz::Decoder d;
    gz::decoder_init(d, body, body_len, cap);
    gz::Token queue[64];
    gz::Batch batch;
    for (uint64_t turns = 8ull * body_len + 2ull; turns; --turns) {
        gz::decode_batch(d, tab, queue, 64, batch);
        for (uint32_t k = 0; k < batch.n; ++k) {
            if (!gz::token_is_match(queue[k])) { out[queue[k].pos] = (uint8_t)queue[k].v; continue; }
            const uint32_t len = gz::token_len(queue[k]), dist = gz::token_dist(queue[k]), pos = queue[k].pos;
            for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[gz::match_src(pos, dist, i)];
        }
        for (uint32_t i = 0; i < batch.stored_len; ++i) out[batch.stored_pos + i] = body[batch.stored_src + i];
        if (d.done || d.status != gz::GZ_OK) break;
    }
    if (d.status != gz::GZ_OK) return d.status;
    if (!d.done) return gz::GZ_TRUNCATED;
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) crc ^= gz::crc_lane_part(crc_tab, out, d.produced, lane, 64);
    return gz::check_trailer(d, crc);
}

// One piece from its start to its landing. sym == nullptr: the count pass, nothing is stored. Otherwise the tokens are executed into
// sym[0, produced): the piece's own range of the scratch, and every store is behind a test against it.
static void run_piece(const uint8_t* body, uint32_t body_len, uint32_t cap, const std::vector<uint64_t>& starts, uint32_t self, gz::Tables& tab, gz::Piece& pc,
                      uint16_t* sym, uint32_t own) {
    gz::PieceDecoder p;
    gz::piece_decoder_init(p, body, body_len, cap, starts.data(), (uint32_t)starts.size(), self, starts[self]);
    gz::Token queue[gz::GZ_PIECE_QUEUE];
    gz::Batch batch;
    bool over = false;
    for (uint64_t turns = 8ull * body_len + 2ull; turns && !over; --turns) {
        gz::piece_decode_batch(p, tab, queue, gz::GZ_PIECE_QUEUE, batch);
        over = p.d.done || p.d.status != gz::GZ_OK;
        if (!sym) continue;
        for (uint32_t k = 0; k < batch.n; ++k) {
            const gz::Token t = queue[k];
            if (!gz::token_is_match(t)) { if (t.pos >= own) die("literal outside the piece's range"); sym[t.pos] = (uint16_t)t.v; continue; }
            const uint32_t len = gz::token_len(t), dist = gz::token_dist(t);
            for (uint32_t i = 0; i < len; ++i) {
                if (t.pos + i >= own) die("match outside the piece's range");
                const int32_t src = gz::piece_match_src(t.pos, dist, i);
                if (src >= (int32_t)(t.pos + i)) die("match source at or behind its position");
                sym[t.pos + i] = src >= 0 ? sym[src] : (uint16_t)(gz::GZ_SYM_MARKER + (uint32_t)(-1 - src));
            }
        }
        for (uint32_t i = 0; i < batch.stored_len; ++i) {
            if (batch.stored_pos + i >= own) die("stored run outside the piece's range");
            sym[batch.stored_pos + i] = body[batch.stored_src + i];
        }
    }
    if (!sym) {
        pc.end_bit = p.end_bit; pc.next = p.landed; pc.produced = p.d.produced;
        pc.status = over ? p.d.status : (int32_t)gz::GZ_TRUNCATED;
        if (pc.status == gz::GZ_OK && p.landed == gz::GZ_PIECE_NONE) pc.status = gz::GZ_PIECE_NO_LANDING;
    } else if (pc.end_bit != p.end_bit || pc.next != p.landed || pc.produced != p.d.produced || p.d.status != gz::GZ_OK) die("the two passes of a piece disagree");
}

// false: the member is handed over
static bool inflate_pieces(const uint8_t* body, uint32_t body_len, uint8_t* out, uint32_t cap, uint32_t piece_bytes, gz::Tables& tab, const uint32_t* crc_tab,
                           std::vector<gz::Piece>& pieces) {
    const uint32_t n = (uint32_t)(((uint64_t)body_len + piece_bytes - 1) / piece_bytes);
    pieces.assign(n, gz::Piece{});
    std::vector<uint64_t> starts(n);
    for (uint32_t i = 0; i < n; ++i) {   // find
        starts[i] = gz::piece_find(body, body_len, piece_bytes, i, tab);
        if (starts[i] != gz::GZ_PIECE_NO_START) { pieces[i].start_bit = starts[i]; pieces[i].flags = gz::PIECE_HAS_START; }
    }
    for (uint32_t i = 0; i < n; ++i) if (pieces[i].flags & gz::PIECE_HAS_START) run_piece(body, body_len, cap, starts, i, tab, pieces[i], nullptr, 0);   // count
    bool complete = gz::piece_chain(pieces.data(), n, body, body_len, cap);
    if (complete) {
        uint16_t* sym = (uint16_t*)malloc(cap ? (size_t)cap * 2 : 2);   // exactly 2 bytes per output byte
        for (uint32_t i = 0; i < n; ++i)
            if (pieces[i].flags & gz::PIECE_LIVE) run_piece(body, body_len, cap, starts, i, tab, pieces[i], sym + pieces[i].out_pos, pieces[i].produced);
        for (uint32_t i = 0; i < n && complete; ++i) {   // windows: live pieces in chain order (the index order)
            const gz::Piece& p = pieces[i];
            if (!(p.flags & gz::PIECE_LIVE)) continue;
            const uint32_t tail = p.produced < gz::GZ_PIECE_WINDOW ? p.produced : gz::GZ_PIECE_WINDOW;
            for (uint32_t j = p.produced - tail; j < p.produced && complete; ++j) complete = gz::piece_resolve_sym(sym[p.out_pos + j], out, p.out_pos, out[p.out_pos + j]);
        }
        uint32_t crc = 0;
        for (uint32_t i = 0; i < n && complete; ++i) {   // resolve
            gz::Piece& p = pieces[i];
            if (!(p.flags & gz::PIECE_LIVE)) continue;
            const uint32_t tail = p.produced < gz::GZ_PIECE_WINDOW ? p.produced : gz::GZ_PIECE_WINDOW;
            for (uint32_t j = 0; j < p.produced - tail && complete; ++j) complete = gz::piece_resolve_sym(sym[p.out_pos + j], out, p.out_pos, out[p.out_pos + j]);
            if (complete) crc ^= gz::crc_mul(gz::crc_bytes(crc_tab, out + p.out_pos, p.produced), gz::crc_xpow8(cap - p.out_pos - p.produced));
        }
        free(sym);
        if (complete) {   // the chain has tested the trailer's place and ISIZE; the CRC is left
            const uint8_t* t = body + body_len - 8;
            complete = ((uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24) == crc;
        }
    }
    if (!complete) for (gz::Piece& p : pieces) p.flags |= gz::PIECE_HANDED;
    return complete;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: test_gz_pieces CASES OUT PIECE_BYTES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    const uint32_t piece_bytes = (uint32_t)strtoul(argv[3], nullptr, 10);
    if (!f || !o) { perror("open"); return 2; }
    if (piece_bytes < 512 || (piece_bytes & (piece_bytes - 1))) return 2;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = gz::crc_table_entry(i);
    gz::Tables* tab = new gz::Tables();
    size_t ok = 0;
    std::vector<gz::Piece> pieces;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        uint8_t* file = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);   // exactly the member: the sanitizer sees a load behind it
        if (hdr[0] && fread(file, 1, hdr[0], f) != hdr[0]) return 2;
        const GzMemberIn m{0, hdr[0], hdr[1]};
        GzPlan plan;
        std::string err;
        if (!gz_plan(file, hdr[0], &m, 1, plan, err)) { fprintf(stderr, "case %u: %s\n", c, err.c_str()); return 2; }
        const GzPlanned& g = plan.members[0];
        int32_t status = g.status;
        uint8_t* out = (uint8_t*)malloc(g.cap ? g.cap : 1);      // exactly the capacity
        pieces.clear();
        if (status == gz::GZ_OK) {
            const bool split = (uint64_t)g.body_len >= 2ull * piece_bytes;
            if (!split || !inflate_pieces(file + g.body, g.body_len, out, g.cap, piece_bytes, *tab, crc_tab, pieces))
                status = inflate_member(file + g.body, g.body_len, out, g.cap, *tab, crc_tab);
        }
        const uint32_t len = status == gz::GZ_OK ? g.cap : 0u, np = (uint32_t)pieces.size();
        fwrite(&status, 4, 1, o);
        fwrite(&len, 4, 1, o);
        if (len) fwrite(out, 1, len, o);
        fwrite(&np, 4, 1, o);
        uint32_t live = 0, dead = 0;
        for (uint32_t i = 0; i < np; ++i) {
            gz::Piece& p = pieces[i];
            p.member = 0;
            fwrite(&p, 32, 1, o);
            live += (p.flags & gz::PIECE_LIVE) != 0;
            dead += (p.flags & gz::PIECE_HAS_START) && !(p.flags & gz::PIECE_LIVE);
            printf("piece %u %u start %llu end %llu produced %u out_pos %u flags %u\n", c, i, (unsigned long long)p.start_bit, (unsigned long long)p.end_bit, p.produced, p.out_pos, p.flags);
        }
        printf("case %u status %d pieces %u live %u dead %u handed %u\n", c, status, np, live, dead, np && (pieces[0].flags & gz::PIECE_HANDED) ? 1u : 0u);
        ok += status == gz::GZ_OK;
        free(out);
        free(file);
    }
    delete tab;
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("gz_pieces ok: %u cases, %zu inflated\n", n, ok);
    return 0;
}
