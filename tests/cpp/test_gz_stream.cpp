// CPU: the rules of stream windows (inflate_core.h "windows of one stream") and the walker of gz_stream.h, driven sequentially through all
// passes the way the kernels of inflate_pieces.hip drive them: find, count (dry), open chain, symbols, windows (the last 32 KiB of every
// live piece, in chain order, piece 0 from the history), resolve (the rest, and the CRC-32 as one part per piece), verdict, new history.
// Built with -fsanitize=address,undefined (tests/test_gz_stream_host.py): every window lives in a heap block of exactly its compressed
// length, symbols and text in blocks of exactly the capacity, the history in one of exactly history_len bytes, so a load outside the
// window or a store outside a piece's own range stops the run.
//
//   test_gz_stream CASES OUT WINDOW_BYTES PIECE_BYTES TEXT_CAP [REF]   CASES: u32 n, then per case u32 len, u32 out_len, bytes (tests/gz_cases.py)
//   test_gz_stream walker                                               the walker's rules and the ISIZE comparison on synthetic numbers
// OUT without REF, per case: u32 n_windows, then per window the record write_window() writes. With REF (a file that holds the true text
// of every case): per case i32 status of the last window, i32 gz_status, u32 n_windows, u32 ended, u64 accepted text bytes, u64 length of
// the common prefix of the accepted text and REF.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gz_plan.h"
#include "gz_stream.h"
#include "inflate_core.h"

using namespace mxy;

static void die(const char* what) { fprintf(stderr, "%s\n", what); exit(3); }

struct Window {
    int32_t status = gz::STREAM_OK, gz_status = gz::GZ_OK;
    uint64_t consumed_bits = 0;   // relative to the window's first byte, header included
    uint32_t text_len = 0, ended = 0, history_markers = 0, cut_by_cap = 0;
    std::vector<gz::Piece> pieces;
};

// One piece from its start to its landing. sym == nullptr: the count pass, nothing is stored.
static void run_piece(const uint8_t* in, uint32_t in_len, uint32_t cap, const std::vector<uint64_t>& starts, uint32_t self, uint32_t history_len, gz::Tables& tab, gz::Piece& pc,
                      uint16_t* sym, uint32_t own) {
    gz::PieceDecoder p;
    gz::stream_piece_decoder_init(p, in, in_len, cap, starts.data(), (uint32_t)starts.size(), self, starts[self], history_len);
    gz::Token queue[gz::GZ_PIECE_QUEUE];
    gz::Batch batch;
    bool over = false;
    for (uint64_t turns = 8ull * in_len + 2ull; turns && !over; --turns) {
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
            sym[batch.stored_pos + i] = in[batch.stored_src + i];
        }
    }
    if (!sym) {
        pc.end_bit = p.end_bit; pc.next = p.landed; pc.produced = p.d.produced;
        pc.status = over ? p.d.status : (int32_t)gz::GZ_TRUNCATED;
        if (pc.status == gz::GZ_OK && p.landed == gz::GZ_PIECE_NONE) pc.status = gz::GZ_PIECE_NO_LANDING;
    } else if (pc.end_bit != p.end_bit || pc.next != p.landed || pc.produced != p.d.produced || p.d.status != gz::GZ_OK) die("the two passes of a piece disagree");
}

// One window: in[0, in_len) with its first block at st.bit. text has text_cap bytes. On STREAM_OK `next` is the state behind the window.
static void run_window(const uint8_t* in, uint32_t in_len, const gz::StreamState& st, const uint8_t* history, uint32_t text_cap, uint32_t piece_bytes, bool file_end,
                       gz::Tables& tab, const uint32_t* crc_tab, uint8_t* text, gz::StreamState& next, Window& w) {
    const uint32_t n = (uint32_t)(((uint64_t)in_len + piece_bytes - 1) / piece_bytes);
    w.pieces.assign(n, gz::Piece{});
    std::vector<uint64_t> starts(n);
    for (uint32_t i = 0; i < n; ++i) {   // find
        starts[i] = gz::stream_piece_find(in, in_len, piece_bytes, i, st.bit, tab);
        if (starts[i] != gz::GZ_PIECE_NO_START) { w.pieces[i].start_bit = starts[i]; w.pieces[i].flags = gz::PIECE_HAS_START; }
    }
    for (uint32_t i = 0; i < n; ++i) if (w.pieces[i].flags & gz::PIECE_HAS_START) run_piece(in, in_len, text_cap, starts, i, st.history_len, tab, w.pieces[i], nullptr, 0);   // count
    const gz::StreamChain c = gz::stream_chain(w.pieces.data(), n, text_cap, file_end);
    if (c.n_live == 0) {
        w.status = c.failed != gz::GZ_OK ? gz::STREAM_FAILED : gz::STREAM_NO_PROGRESS;
        w.gz_status = c.failed;
        return;
    }
    if (!c.ended) {   // was it the capacity that stopped the chain, and not the input's end?
        const gz::Piece& stop = w.pieces[w.pieces[c.last].next];
        w.cut_by_cap = (stop.flags & gz::PIECE_HAS_START) && stop.status == gz::GZ_OK && (uint64_t)c.text_len + stop.produced > text_cap;
    }
    uint16_t* sym = (uint16_t*)malloc(text_cap ? (size_t)text_cap * 2 : 2);   // exactly 2 bytes per byte of capacity
    for (uint32_t i = 0; i < n; ++i)
        if (w.pieces[i].flags & gz::PIECE_LIVE) run_piece(in, in_len, text_cap, starts, i, st.history_len, tab, w.pieces[i], sym + w.pieces[i].out_pos, w.pieces[i].produced);
    bool ok = true;
    for (uint32_t i = 0; i < n && ok; ++i) {   // windows: live pieces in chain order (the index order)
        const gz::Piece& p = w.pieces[i];
        if (!(p.flags & gz::PIECE_LIVE)) continue;
        const uint32_t tail = p.produced < gz::GZ_PIECE_WINDOW ? p.produced : gz::GZ_PIECE_WINDOW;
        for (uint32_t j = p.produced - tail; j < p.produced && ok; ++j) {
            const uint16_t s = sym[p.out_pos + j];
            ok = gz::stream_resolve_sym(s, text, p.out_pos, history, st.history_len, text[p.out_pos + j]);
            if (i == 0 && s >= gz::GZ_SYM_MARKER) ++w.history_markers;
        }
    }
    uint32_t crc = 0;
    for (uint32_t i = 0; i < n && ok; ++i) {   // resolve
        gz::Piece& p = w.pieces[i];
        if (!(p.flags & gz::PIECE_LIVE)) continue;
        const uint32_t tail = p.produced < gz::GZ_PIECE_WINDOW ? p.produced : gz::GZ_PIECE_WINDOW;
        for (uint32_t j = 0; j < p.produced - tail && ok; ++j) {
            const uint16_t s = sym[p.out_pos + j];
            ok = gz::stream_resolve_sym(s, text, p.out_pos, history, st.history_len, text[p.out_pos + j]);
            if (i == 0 && s >= gz::GZ_SYM_MARKER) ++w.history_markers;
        }
        if (ok) crc ^= gz::stream_piece_crc(gz::crc_bytes(crc_tab, text + p.out_pos, p.produced), c.text_len, p.out_pos, p.produced);
    }
    free(sym);
    // verdict
    if (!ok) { w.status = gz::STREAM_FAILED; w.gz_status = gz::GZ_BAD_DISTANCE; w.history_markers = 0; return; }
    const uint32_t all_crc = gz::stream_crc_combine(st.crc, crc, c.text_len);
    if (c.ended) {
        const int32_t e = gz::stream_end_check(in, in_len, c.consumed_bits, st.text_bytes, c.text_len, all_crc);
        if (e != gz::GZ_OK) { w.status = gz::STREAM_FAILED; w.gz_status = e; return; }
    }
    w.consumed_bits = c.consumed_bits; w.text_len = c.text_len; w.ended = c.ended;
    next.text_bytes = st.text_bytes + c.text_len; next.crc = all_crc; next.bit = (uint32_t)(c.consumed_bits & 7u);
    next.history_len = gz::stream_history_len(st.history_len, c.text_len);
    for (uint32_t j = 0; j < next.history_len; ++j) next.history[j] = gz::stream_history_byte(history, st.history_len, text, c.text_len, next.history_len, j);
}

static void put(FILE* o, const void* p, size_t n) { if (n && fwrite(p, 1, n, o) != n) die("write"); }
template <class T> static void put(FILE* o, T v) { put(o, &v, sizeof v); }

// i32 status, i32 gz_status, u64 consumed_bits, u32 text_len, u32 ended, u32 flags, u32 bit (of the window's first block), u64 offset, u64 len
// (of the window in the file), u64 base_bit (the file's bit that piece bits count from), u32 history_markers, u32 cut_by_cap; the state
// behind the window: u64 text_bytes, u32 crc, u32 bit, u32 history_len, history_len bytes; text_len bytes; u32 n_pieces, 32 bytes each.
static void write_window(FILE* o, const Window& w, const GzStreamWindow& gw, uint64_t base_bit, const gz::StreamState& next, const uint8_t* text) {
    put(o, w.status); put(o, w.gz_status); put(o, w.consumed_bits); put(o, w.text_len); put(o, w.ended); put(o, gw.flags); put(o, gw.bit);
    put(o, gw.offset); put(o, gw.len); put(o, base_bit); put(o, w.history_markers); put(o, w.cut_by_cap);
    put(o, next.text_bytes); put(o, next.crc); put(o, next.bit); put(o, next.history_len);
    put(o, next.history, next.history_len);
    put(o, text, w.text_len);
    put(o, (uint32_t)w.pieces.size());
    for (const gz::Piece& p : w.pieces) put(o, &p, 32);
}

static int walker_selftest() {
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { printf("FAIL %s\n", what); ++bad; } };
    {   // the first window: the fixed guess, FIRST, and the rest of a short file with FILE_END
        GzStreamWalker w(1000000, 65536, 4096, 1 << 20);
        GzStreamWindow a = w.next();
        expect(a.offset == 0 && a.len == 65536 && a.bit == 0 && a.flags == GZ_STREAM_FIRST, "first window");
        // 50 000 bytes and 5 bits consumed for 400 000 bytes of text: 8 : 1
        expect(w.accept(a, 50000ull * 8 + 5, 400000, false) && !w.over, "accept");
        expect(w.at == 50000 && w.bit == 5 && w.text_bytes == 400000, "next start");
        // 2^20 / 8 = 131072, an eighth more and a piece: above window_bytes, so window_bytes
        GzStreamWindow b = w.next();
        expect(b.offset == 50000 && b.bit == 5 && b.len == 65536 && b.flags == 0, "clamped above");
        expect(w.accept(b, 60000ull * 8, 60000, false), "accept 2");   // 1 : 1 now: 2^20 bytes wanted, still clamped
        expect(w.at == 110000 && w.bit == 0 && w.next().len == 65536, "byte aligned");
        GzStreamWalker s(80000, 65536, 4096, 1 << 20);
        expect(s.next().len == 80000 && s.next().flags == (GZ_STREAM_FIRST | GZ_STREAM_FILE_END), "a rest of less than a quarter joins the window");
        GzStreamWalker t(81921, 65536, 4096, 1 << 20);
        expect(t.next().len == 65536 && t.next().flags == GZ_STREAM_FIRST, "a rest of more than a quarter does not");
    }
    {   // the ratio: 1000 compressed bytes gave 100 000 bytes of text, the capacity is 50 000: 500 + 62 + 512, no less than four pieces
        GzStreamWalker w(1 << 30, 1 << 20, 512, 50000);
        GzStreamWindow a = w.next();
        expect(w.accept(a, 8000, 100000, false), "accept 3");
        expect(w.want == 2048 && w.next().len == 2048, "clamped below");
        GzStreamWindow b = w.next();
        expect(w.accept(b, 2000 * 8, 25000, false) && w.want == 4000 + 500 + 512, "ratio followed");
        GzStreamWindow c = w.next();
        expect(c.offset == 3000 && w.accept(c, 4000 * 8 + 1, 50000, true) && w.over && w.ended && w.windows == 3, "ended");
    }
    {   // a device that claims nothing consumed, or more than it was given, ends the chain
        GzStreamWalker w(1 << 20, 65536, 4096, 1 << 20);
        GzStreamWindow a = w.next();
        a.bit = 3;
        GzStreamWalker x = w, y = w;
        expect(!x.accept(a, 3, 10, false) && x.over && !x.ended, "no progress in bits");
        expect(!y.accept(a, 65536ull * 8 + 1, 10, false) && y.over, "beyond the window");
        w.refuse();
        expect(w.over && !w.ended && w.windows == 1, "refuse");
        expect(GzStreamWalker(0, 65536, 4096, 1).over, "empty file");
    }
    // ISIZE is the length modulo 2^32
    expect(gz::stream_isize(0xFFFFFFF0ull, 15) == 0xFFFFFFFFu, "just below 2^32");
    expect(gz::stream_isize(0xFFFFFFF0ull, 16) == 0u && gz::stream_isize(0xFFFFFFF0ull, 17) == 1u, "just above 2^32");
    expect(gz::stream_isize(3ull << 32 | 7u, 0xFFFFFFF9u) == 0u && gz::stream_isize(1ull << 32, 5) == 5u, "several times 2^32");
    {
        uint8_t tr[8] = {0x78, 0x56, 0x34, 0x12, 1, 0, 0, 0};
        expect(gz::stream_end_check(tr, 8, 0, 0xFFFFFFF0ull, 17, 0x12345678u) == gz::GZ_OK, "trailer above 2^32");
        expect(gz::stream_end_check(tr, 8, 0, 0xFFFFFFF0ull, 16, 0x12345678u) == gz::GZ_SIZE_MISMATCH, "size");
        expect(gz::stream_end_check(tr, 8, 0, 0xFFFFFFF0ull, 17, 0x12345679u) == gz::GZ_CRC_MISMATCH, "crc");
        expect(gz::stream_end_check(tr, 7, 0, 0xFFFFFFF0ull, 17, 0x12345678u) == gz::GZ_TRUNCATED, "truncated");
        uint8_t more[10] = {0, 0x78, 0x56, 0x34, 0x12, 1, 0, 0, 0, 9};
        expect(gz::stream_end_check(more, 10, 3, 0xFFFFFFF0ull, 17, 0x12345678u) == gz::GZ_TRAILING_DATA, "trailing data");
        expect(gz::stream_end_check(more, 10, 3, 0xFFFFFFF0ull, 16, 0x12345678u) == gz::GZ_SIZE_MISMATCH, "size in front of trailing data");
    }
    expect(gz::stream_state_valid(5, 7, 5) && !gz::stream_state_valid(5, 8, 5) && !gz::stream_state_valid(5, 0, 6) && !gz::stream_state_valid(1 << 20, 0, 32769), "state");
    printf(bad ? "gz_stream walker FAILED\n" : "gz_stream walker ok\n");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "walker")) return walker_selftest();
    if (argc != 6 && argc != 7) { fprintf(stderr, "usage: test_gz_stream CASES OUT WINDOW_BYTES PIECE_BYTES TEXT_CAP [REF] | walker\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    const uint32_t window_bytes = (uint32_t)strtoul(argv[3], nullptr, 10), piece_bytes = (uint32_t)strtoul(argv[4], nullptr, 10), text_cap = (uint32_t)strtoul(argv[5], nullptr, 10);
    if (!f || !o) { perror("open"); return 2; }
    if (!gz_piece_bytes_valid(piece_bytes) || window_bytes < piece_bytes || !text_cap) return 2;
    std::vector<uint8_t> ref;
    if (argc == 7) {
        FILE* r = fopen(argv[6], "rb");
        if (!r) { perror("open"); return 2; }
        uint8_t buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof buf, r)) != 0;) ref.insert(ref.end(), buf, buf + k);
        fclose(r);
    }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = gz::crc_table_entry(i);
    gz::Tables* tab = new gz::Tables();
    gz::StreamState* st = new gz::StreamState();
    gz::StreamState* nx = new gz::StreamState();
    size_t whole = 0, total_windows = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        std::vector<uint8_t> file(hdr[0]);
        if (hdr[0] && fread(file.data(), 1, hdr[0], f) != hdr[0]) return 2;
        GzStreamWalker walk(file.size(), window_bytes, piece_bytes, text_cap);
        memset(st, 0, sizeof *st);
        uint8_t* text = (uint8_t*)malloc(text_cap);   // exactly the capacity
        uint32_t n_windows = 0;
        uint64_t accepted = 0, common = 0;
        bool diverged = false;
        Window last;
        long count_at = 0;
        if (ref.empty()) { count_at = ftell(o); put(o, (uint32_t)0); }
        while (!walk.over) {
            const GzStreamWindow gw = walk.next();
            Window w;
            uint64_t body = 0;
            if (gw.flags & GZ_STREAM_FIRST) {   // the header is the host's
                if (gz_parse_header(file.data() + gw.offset, gw.len, body) != GZ_PLAN_OK) { w.status = gz::STREAM_FAILED; w.gz_status = gz::GZ_BAD_HEADER; }
            }
            const uint32_t in_len = (uint32_t)(gw.len - body);
            uint8_t* in = (uint8_t*)malloc(in_len ? in_len : 1);   // exactly the window: the sanitizer sees a load outside it
            memcpy(in, file.data() + gw.offset + body, in_len);
            uint8_t* history = (uint8_t*)malloc(st->history_len ? st->history_len : 1);   // exactly the history
            memcpy(history, st->history, st->history_len);
            *nx = *st;
            if (w.status == gz::STREAM_OK) {
                if (in_len == 0) w.status = gz::STREAM_NO_PROGRESS;
                else run_window(in, in_len, *st, history, text_cap, piece_bytes, (gw.flags & GZ_STREAM_FILE_END) != 0, *tab, crc_tab, text, *nx, w);
            }
            if (w.status == gz::STREAM_OK) w.consumed_bits += body * 8u;
            else { w.consumed_bits = 0; w.text_len = 0; w.ended = 0; }
            ++n_windows;
            if (ref.empty()) write_window(o, w, gw, (gw.offset + body) * 8u, *nx, text);
            else if (w.status == gz::STREAM_OK) {
                for (uint32_t j = 0; j < w.text_len; ++j) {
                    if (!diverged && accepted + j < ref.size() && ref[accepted + j] == text[j]) ++common; else diverged = true;
                }
                accepted += w.text_len;
            }
            uint32_t live = 0;
            for (const gz::Piece& p : w.pieces) live += (p.flags & gz::PIECE_LIVE) != 0;
            if (ref.empty())
                printf("window %u %u offset %llu len %llu bit %u flags %u status %d gz %d consumed %llu text %u ended %u pieces %zu live %u history_markers %u cut_by_cap %u\n", c, n_windows - 1,
                       (unsigned long long)gw.offset, (unsigned long long)gw.len, gw.bit, gw.flags, w.status, w.gz_status, (unsigned long long)w.consumed_bits, w.text_len, w.ended,
                       w.pieces.size(), live, w.history_markers, w.cut_by_cap);
            free(in);
            free(history);
            if (w.status == gz::STREAM_OK) {
                if (!walk.accept(gw, w.consumed_bits, w.text_len, w.ended != 0)) die("an OK window that the walker does not accept");
                *st = *nx;
            } else walk.refuse();
            last = std::move(w);
        }
        if (ref.empty()) {
            const long end = ftell(o);
            fseek(o, count_at, SEEK_SET); put(o, n_windows); fseek(o, end, SEEK_SET);
        } else {
            put(o, last.status); put(o, last.gz_status); put(o, n_windows); put(o, (uint32_t)walk.ended); put(o, accepted); put(o, common);
        }
        whole += walk.ended;
        total_windows += n_windows;
        free(text);
    }
    delete tab; delete st; delete nx;
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("gz_stream ok: %u cases, %zu windows, %zu chains reached the stream's end\n", n, total_windows, whole);
    return 0;
}
