// CPU check of matchy_amd/csrc/batch_reader.h: the one newline cut rule, the stream batcher against it, and the inner page range.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I matchy_amd/csrc tests/cpp/test_batch_reader.cpp -o /tmp/test_batch_reader
// (no library: nothing here calls prefault_and_pin, so matchy_amd_host_register is not needed at link time)
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "batch_reader.h"

using namespace mxy;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the ends of all batches of buf under the mapped rule, with the properties every caller relies on
static std::vector<size_t> cuts_of(const std::vector<uint8_t>& buf, size_t bb, int id) {
    std::vector<size_t> ends;
    for (size_t pos = 0; pos < buf.size();) {
        const size_t end = newline_cut(buf.data(), pos, buf.size(), bb);
        CHECK(end > pos && end <= buf.size(), "case %d: batch [%zu, %zu) of %zu", id, pos, end, buf.size());
        if (end <= pos || end > buf.size()) break;
        if (end != buf.size()) CHECK(buf[end - 1] == '\n', "case %d: batch ending at %zu is not the last and does not end a line", id, end);
        if (end - pos > bb)   // longer than a batch: exactly one line (no '\n' before its last byte)
            CHECK(memchr(buf.data() + pos, '\n', end - pos - 1) == nullptr, "case %d: batch [%zu, %zu) exceeds %zu bytes with several lines", id, pos, end, bb);
        ends.push_back(end);
        pos = end;
    }
    CHECK(ends.empty() ? buf.empty() : ends.back() == buf.size(), "case %d: batches do not cover the input", id);   // contiguous from 0: they concatenate to it
    return ends;
}

int main() {
    std::mt19937 rng(20240607);
    auto upto = [&](size_t n) { return (size_t)(rng() % (n + 1)); };
    int cases = 0;
    for (int round = 0; round < 6000; ++round) {
        const size_t bb = round % 7 == 0 ? 1 + upto(3) : 1 + upto(63);
        size_t n = upto(400);
        const int shape = round % 8;
        if (shape == 0) n = 0;                                   // empty
        if (shape == 5) n = bb * (1 + upto(6));                  // length an exact multiple of the batch
        std::vector<uint8_t> buf(n);
        // 1: no newline at all, 2: only newlines, 3: lines longer than several batches, else a mix with short and long lines
        const unsigned nl_one_in = shape == 3 ? (unsigned)(bb * (2 + upto(4))) : shape == 4 ? 2u : 3u + (unsigned)upto(20);
        for (uint8_t& c : buf) c = shape == 1 ? 'a' : shape == 2 ? '\n' : rng() % nl_one_in == 0 ? '\n' : (uint8_t)('a' + rng() % 8);
        const std::vector<size_t> want = cuts_of(buf, bb, round);

        // the stream batcher over the same bytes, through a reader that returns random short counts and now and then EINTR
        size_t fed = 0, eintrs = 0;
        auto rd = [&](void* dst, size_t room) -> ssize_t {
            if (room == 0) { CHECK(false, "case %d: read of 0 bytes asked for", round); errno = EINVAL; return -1; }
            if (rng() % 9 == 0) { ++eintrs; errno = EINTR; return -1; }
            size_t k = std::min(room, buf.size() - fed);
            if (k) k = 1 + upto(std::min<size_t>(k, round % 3 ? 50 : 5) - 1);
            if (k) memcpy(dst, buf.data() + fed, k);
            fed += k;
            return (ssize_t)k;
        };
        std::vector<size_t> got;
        std::vector<uint8_t> joined;
        uint64_t expect_off = 0;
        const StreamEnd e = read_batches(rd, bb, [&](Bytes&& b, size_t len, uint64_t off) {
            CHECK(off == expect_off, "case %d: batch offset %llu, expected %llu", round, (unsigned long long)off, (unsigned long long)expect_off);
            memset(b.get() + len, 0x5A, 16);   // the spare bytes behind a batch are the caller's to write (the sanitizer checks the room)
            joined.insert(joined.end(), b.get(), b.get() + len);
            expect_off += len;
            got.push_back((size_t)expect_off);
            return true;
        });
        CHECK(e == StreamEnd::DONE, "case %d: stream ended with %d", round, (int)e);
        CHECK(joined == buf, "case %d: the stream's batches do not concatenate to the input", round);
        CHECK(got == want, "case %d (batch %zu, %zu bytes): %zu stream batches, %zu mapped", round, bb, n, got.size(), want.size());
        ++cases;
    }
    {   // a sink that stops, and a reader that fails: reported as such, nothing handed out afterwards
        const std::vector<uint8_t> buf(100, '\n');
        size_t fed = 0, seen = 0;
        auto rd = [&](void* dst, size_t room) -> ssize_t { const size_t k = std::min(room, buf.size() - fed); if (k) memcpy(dst, buf.data() + fed, k); fed += k; return (ssize_t)k; };
        CHECK(read_batches(rd, 10, [&](Bytes&&, size_t, uint64_t) { return ++seen < 3; }) == StreamEnd::STOPPED && seen == 3, "stopping sink: %zu batches", seen);
        seen = 0;
        auto failing = [&](void*, size_t) -> ssize_t { errno = EIO; return -1; };
        CHECK(read_batches(failing, 10, [&](Bytes&&, size_t, uint64_t) { ++seen; return true; }) == StreamEnd::FAILED && seen == 0 && errno == EIO, "failing reader");
    }
    // inner_pages: unaligned ranges shorter and longer than a page, against the definition (every whole page inside, nothing else)
    for (int round = 0; round < 4000; ++round) {
        const uintptr_t p = ((uintptr_t)1 << 32) + upto(3 * 4096);
        const size_t n = round % 4 == 0 ? upto(4095) : round % 4 == 1 ? 4096 + upto(5 * 4096) : round % 4 == 2 ? 4096 * upto(3) : upto(9000);
        uintptr_t a = 1, b = 2;
        const bool any = inner_pages((const void*)p, n, a, b);
        bool want_any = false;
        for (uintptr_t page = (p & ~(uintptr_t)4095) - 4096; page <= p + n + 4096; page += 4096) {
            const bool inside = page >= p && page + 4096 <= p + n;
            want_any = want_any || inside;
            if (any) CHECK(inside == (page >= a && page + 4096 <= b), "inner_pages(%#zx, %zu): page %#zx", (size_t)p, n, (size_t)page);
        }
        CHECK(any == want_any, "inner_pages(%#zx, %zu) = %d", (size_t)p, n, (int)any);
        if (any) CHECK(a % 4096 == 0 && b % 4096 == 0 && a >= p && b <= p + n && a - p < 4096 && p + n - b < 4096, "inner_pages(%#zx, %zu) = [%#zx, %#zx)", (size_t)p, n, (size_t)a, (size_t)b);
    }
    if (bad) { printf("batch_reader: %d failures\n", bad); return 1; }
    printf("batch_reader ok: %d buffers\n", cases);
    return 0;
}
