// CPU check of matchy_amd/csrc/utf16_core.h and of the 16-bit cut rule of csrc/batch_reader.h.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I matchy_amd/csrc tests/cpp/test_utf16.cpp -o /tmp/test_utf16
//   test_utf16 cases IN OUT   transcodes every case of IN (tests/utf16_cases.py write_case_file) tile by tile, the way the kernels
//                             partition the work: tile_count of every tile, an exclusive prefix, then tile_write of every tile into
//                             its own range of a buffer of exactly the total (a pass that disagrees with the other stops the sanitized
//                             program or fails the check). OUT: per case u32 length, u32 U+FFFD written, the bytes.
//   test_utf16 cuts           newline_cut16 and read_batches16 on constructed and random inputs
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "batch_reader.h"
#include "utf16_core.h"

using namespace mxy;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static int run_cases(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    FILE* o = fopen(out_path, "wb");
    if (!f || !o) { printf("cannot open files\n"); return 2; }
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 2;
        const uint32_t order = head[0], len = head[1];
        std::vector<uint8_t> data(len);   // exactly len bytes: a read behind the input stops the program
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        const uint64_t n_tiles = utf16::tiles(len);
        std::vector<uint32_t> prefix(n_tiles + 1, 0);
        uint64_t replaced = 0;
        for (uint64_t t = 0; t < n_tiles; ++t) {
            const uint32_t k = utf16::tile_count(data.data(), len, order, t, &replaced);
            CHECK(k <= utf16::TILE_OUT_MAX, "case %u tile %llu: %u bytes", c, (unsigned long long)t, k);
            prefix[t + 1] = prefix[t] + k;
        }
        const uint32_t total = prefix[n_tiles];
        CHECK(total <= utf16::out_bound(len), "case %u: %u bytes from %u", c, total, len);
        std::vector<uint8_t> text(total);
        for (uint64_t t = 0; t < n_tiles; ++t) {
            uint8_t tile[utf16::TILE_OUT_MAX];
            const uint32_t k = utf16::tile_write(data.data(), len, order, t, tile);
            CHECK(k == prefix[t + 1] - prefix[t], "case %u tile %llu: the write pass gives %u bytes, the count pass %u", c, (unsigned long long)t, k, prefix[t + 1] - prefix[t]);
            if (k != prefix[t + 1] - prefix[t]) return 1;
            if (k) memcpy(text.data() + prefix[t], tile, k);
        }
        const uint32_t rep32 = (uint32_t)replaced;
        fwrite(&total, 4, 1, o); fwrite(&rep32, 4, 1, o);
        if (total) fwrite(text.data(), 1, total, o);
    }
    fclose(f); fclose(o);
    if (!bad) printf("utf16 cases ok: %u\n", n_cases);
    return bad ? 1 : 0;
}

static std::vector<uint8_t> units(std::initializer_list<uint32_t> u, uint32_t order) {
    std::vector<uint8_t> b;
    for (uint32_t x : u) { if (order) { b.push_back(x >> 8); b.push_back(x & 0xFF); } else { b.push_back(x & 0xFF); b.push_back(x >> 8); } }
    return b;
}

// the rule read forward, unit by unit: the last line end inside the window, else the first one behind it, else the end
static size_t naive_cut16(const std::vector<uint8_t>& buf, size_t pos, size_t bb, uint32_t order) {
    auto nl = [&](size_t i) { return buf[i + (order ? 1 : 0)] == 0x0A && buf[i + (order ? 0 : 1)] == 0x00; };
    if (buf.size() - pos <= bb) return buf.size();
    size_t best = 0, i = pos;
    for (; i + 2 <= pos + bb; i += 2) if (nl(i)) best = i + 2;
    if (best) return best;
    for (; i + 2 <= buf.size(); i += 2) if (nl(i)) return i + 2;
    return buf.size();
}

// the ends of all batches of buf under newline_cut16, with the properties the callers rely on
static std::vector<size_t> cuts_of(const std::vector<uint8_t>& buf, size_t bb, uint32_t order, int id) {
    std::vector<size_t> ends;
    for (size_t pos = 0; pos < buf.size();) {
        const size_t end = newline_cut16(buf.data(), pos, buf.size(), bb, order);
        CHECK(end > pos && end <= buf.size(), "case %d: batch [%zu, %zu) of %zu", id, pos, end, buf.size());
        if (end <= pos || end > buf.size()) break;
        if (end != buf.size()) {
            CHECK(end % 2 == 0, "case %d: cut at the odd offset %zu", id, end);
            CHECK(end >= 2 && is_newline16(buf.data() + end - 2, order), "case %d: batch ending at %zu is not the last and does not end a line", id, end);
        }
        CHECK(end == naive_cut16(buf, pos, bb, order), "case %d: batch [%zu, %zu), the rule read forward gives %zu", id, pos, end, naive_cut16(buf, pos, bb, order));
        ends.push_back(end);
        pos = end;
    }
    CHECK(ends.empty() ? buf.empty() : ends.back() == buf.size(), "case %d: batches do not cover the input", id);
    return ends;
}

static int run_cuts() {
    for (uint32_t order = 0; order < 2; ++order) {
        {   // 0A as the other byte of a unit (U+0A41) is no cut; the 000A behind it is
            const std::vector<uint8_t> b = units({0x0A41, 0x0A41, 0x0A41, 0x000A, 0x0041, 0x0041}, order);
            CHECK(newline_cut16(b.data(), 0, b.size(), 6, order) == 8, "U+0A41: cut at %zu", newline_cut16(b.data(), 0, b.size(), 6, order));
            CHECK(newline_cut16(b.data(), 0, b.size(), 10, order) == 8, "U+0A41, window over the line end");
        }
        {   // 00 0A at an odd offset inside xx00 0Ayy is no cut
            const std::vector<uint8_t> b = order ? units({0x4100, 0x0A42, 0x4100, 0x0A42, 0x000A, 0x0043}, 1) : units({0x0A41, 0x4200, 0x0A41, 0x4200, 0x000A, 0x0043}, 0);
            const void* odd = memmem(b.data(), b.size(), order ? "\x00\x0A" : "\x0A\x00", 2);
            CHECK(odd && ((const uint8_t*)odd - b.data()) % 2 == 1, "the case holds a line end's bytes at an odd offset");
            CHECK(newline_cut16(b.data(), 0, b.size(), 4, order) == 10, "odd offset: cut at %zu", newline_cut16(b.data(), 0, b.size(), 4, order));
            CHECK(newline_cut16(b.data(), 0, b.size(), 9, order) == 10, "odd offset, odd window");
        }
        {   // a line longer than the window, then a short one; a window that ends inside a unit
            const std::vector<uint8_t> b = units({0x41, 0x42, 0x43, 0x44, 0x45, 0x0A, 0x46, 0x0A, 0x47}, order);
            CHECK(newline_cut16(b.data(), 0, b.size(), 4, order) == 12, "long line");
            CHECK(newline_cut16(b.data(), 0, b.size(), 11, order) == 12, "the line end straddles the window's end: it is not inside");
            CHECK(newline_cut16(b.data(), 0, b.size(), 12, order) == 12, "the line end is the window's last unit");
            CHECK(newline_cut16(b.data(), 12, b.size(), 4, order) == 16, "second batch");
            CHECK(newline_cut16(b.data(), 16, b.size(), 4, order) == 18, "rest");
            std::vector<uint8_t> o = b;
            o.push_back(0x0A);   // an odd last byte is the input's last
            CHECK(newline_cut16(o.data(), 16, o.size(), 2, order) == o.size(), "odd last byte");
        }
    }
    std::mt19937 rng(20260102);
    auto upto = [&](size_t n) { return (size_t)(rng() % (n + 1)); };
    int cases = 0;
    for (int round = 0; round < 6000; ++round) {
        const uint32_t order = round & 1;
        const size_t bb = round % 7 == 0 ? 1 + upto(3) : 1 + upto(63);
        size_t n = upto(400);
        const int shape = round % 8;
        if (shape == 0) n = 0;
        if (shape == 5) n = bb * (1 + upto(6));
        std::vector<uint8_t> buf(n);
        // 1: no line end, 2: only line ends, 3: lines longer than several windows, 6: bytes 00 and 0A at random (line ends' bytes at odd
        // offsets and as halves of other units), else a mix
        const unsigned nl_one_in = shape == 3 ? (unsigned)(bb * (2 + upto(4))) : shape == 4 ? 2u : 3u + (unsigned)upto(20);
        for (size_t i = 0; i + 1 < n; i += 2) {
            uint32_t x = shape == 1 ? 0x61 : shape == 2 ? 0x0A : rng() % nl_one_in == 0 ? 0x0A : rng() % 5 == 0 ? (rng() % 2 ? 0x0A41 : 0x410A) : 0x61 + rng() % 8;
            buf[i] = order ? x >> 8 : x & 0xFF; buf[i + 1] = order ? x & 0xFF : x >> 8;
        }
        if (shape == 6) for (uint8_t& c : buf) c = rng() % 2 ? 0x00 : 0x0A;
        if (n & 1) buf[n - 1] = rng() % 2 ? 0x0A : 0x00;
        const std::vector<size_t> want = cuts_of(buf, bb, order, round);
        // the reader over the same bytes: reads of random short counts, every third round one byte at a time
        size_t fed = 0;
        auto rd = [&](void* dst, size_t room) -> ssize_t {
            if (room == 0) { CHECK(false, "case %d: read of 0 bytes asked for", round); errno = EINVAL; return -1; }
            if (rng() % 9 == 0) { errno = EINTR; return -1; }
            size_t k = std::min(room, buf.size() - fed);
            if (k) k = round % 3 == 0 ? 1 : 1 + upto(std::min<size_t>(k, 50) - 1);
            if (k) memcpy(dst, buf.data() + fed, k);
            fed += k;
            return (ssize_t)k;
        };
        std::vector<size_t> got;
        std::vector<uint8_t> joined;
        uint64_t expect_off = 0;
        const StreamEnd e = read_batches16(rd, bb, order, [&](Bytes&& b, size_t len, uint64_t off) {
            CHECK(off == expect_off, "case %d: batch offset %llu, expected %llu", round, (unsigned long long)off, (unsigned long long)expect_off);
            memset(b.get() + len, 0x5A, 16);   // the spare bytes behind a batch are the caller's to write
            joined.insert(joined.end(), b.get(), b.get() + len);
            expect_off += len;
            got.push_back((size_t)expect_off);
            return true;
        });
        CHECK(e == StreamEnd::DONE, "case %d: stream ended with %d", round, (int)e);
        CHECK(joined == buf, "case %d: the stream's batches do not concatenate to the input", round);
        CHECK(got == want, "case %d (window %zu, %zu bytes): %zu stream batches, %zu from the whole buffer", round, bb, n, got.size(), want.size());
        ++cases;
    }
    if (!bad) printf("utf16 cuts ok: %d\n", cases);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "cases")) return run_cases(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "cuts")) return run_cuts();
    printf("usage: test_utf16 cases IN OUT | test_utf16 cuts\n");
    return 2;
}
