// Host side of feeding a scan: where a buffer is cut into batches, how a stream becomes owned batches, and which pages of a batch are
// faulted in and pinned ahead of its copy. Host only (no HIP include) and header-only: the command line is a translation unit of its
// own linked against the library, and the unit test builds this file with nothing else.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>

#include <sys/mman.h>

#include "../../include/matchy_amd.h"

namespace mxy {

// THE cut rule. The batch that starts at `pos` of base[0, size) ends at the returned offset: the window is batch_bytes long; if input
// lies behind it the batch ends behind the window's last '\n', or — a line longer than the window — behind that line's end, or at
// `size` when no '\n' follows. Every batch but the last ends in '\n', and a batch longer than batch_bytes is exactly one line.
inline size_t newline_cut(const uint8_t* base, size_t pos, size_t size, size_t batch_bytes) {
    if (size - pos <= batch_bytes) return size;
    const size_t end = pos + batch_bytes;
    if (const void* nl = memrchr(base + pos, '\n', end - pos)) return (size_t)((const uint8_t*)nl - base) + 1;
    const void* fw = memchr(base + end, '\n', size - end);
    return fw ? (size_t)((const uint8_t*)fw - base) + 1 : size;
}

// The same rule over UTF-16 code units (byte_order: MATCHY_UTF16_LE / _BE): base[0] is the first byte of the stream that is transcoded
// and `pos` is even, so units lie at even offsets. A batch ends behind a 000A unit: the window's last one that lies inside it as a
// whole, or — a line longer than the window — the first one behind those, or at `size`. '\n' is no surrogate, so no pair and no line
// spans two batches; every cut but `size` is even, and an odd last byte can only be the input's last. A 0A that is the other byte
// of a unit (U+0A41), or a 00 0A at an odd offset (xx00 0Ayy), is no line end.
inline bool is_newline16(const uint8_t* u, uint32_t byte_order) { return u[byte_order ? 1 : 0] == '\n' && u[byte_order ? 0 : 1] == 0; }
// offset behind the last 000A unit that lies in b[0, n) as a whole, 0: none
inline size_t last_newline16(const uint8_t* b, size_t n, uint32_t byte_order) {
    for (size_t i = n & ~(size_t)1; i >= 2; i -= 2)
        if (is_newline16(b + i - 2, byte_order)) return i;
    return 0;
}
// offset behind the first 000A unit that starts at or behind `from` (rounded down to a unit) and lies in b[0, n) as a whole, 0: none
inline size_t first_newline16(const uint8_t* b, size_t from, size_t n, uint32_t byte_order) {
    for (size_t i = from & ~(size_t)1; i + 2 <= n; i += 2)
        if (is_newline16(b + i, byte_order)) return i + 2;
    return 0;
}
inline size_t newline_cut16(const uint8_t* base, size_t pos, size_t size, size_t batch_bytes, uint32_t byte_order) {
    if (size - pos <= batch_bytes) return size;
    if (const size_t k = last_newline16(base + pos, batch_bytes, byte_order)) return pos + k;
    const size_t k = first_newline16(base + pos, batch_bytes, size - pos, byte_order);
    return k ? pos + k : size;
}

// What read_batches needs of a cut rule, over a buffer that starts at a batch's first byte. whole: the cut of b[0, have) when nothing
// follows it; last: the offset behind the last line end inside the window b[0, n), 0 = none; first: behind the first line end at or
// behind `from`, 0 = none in b[0, n) yet.
struct CutBytes {
    size_t whole(const uint8_t* b, size_t have, size_t batch_bytes) const { return newline_cut(b, 0, have, batch_bytes); }
    size_t last(const uint8_t* b, size_t n) const { const void* nl = memrchr(b, '\n', n); return nl ? (size_t)((const uint8_t*)nl - b) + 1 : 0; }
    size_t first(const uint8_t* b, size_t from, size_t n) const { const void* nl = memchr(b + from, '\n', n - from); return nl ? (size_t)((const uint8_t*)nl - b) + 1 : 0; }
};
struct CutUnits16 {
    uint32_t byte_order;
    size_t whole(const uint8_t* b, size_t have, size_t batch_bytes) const { return newline_cut16(b, 0, have, batch_bytes, byte_order); }
    size_t last(const uint8_t* b, size_t n) const { return last_newline16(b, n, byte_order); }
    size_t first(const uint8_t* b, size_t from, size_t n) const { return first_newline16(b, from, n, byte_order); }
};

// malloc'ed bytes (no value-initialisation: a 256 MiB batch buffer would be zeroed before every read; realloc grows it for a long
// line). Whoever takes a batch from the reader owns it; across the C ABI it travels as release() and comes back through free().
struct FreeBytes { void operator()(uint8_t* p) const { free(p); } };
using Bytes = std::unique_ptr<uint8_t[], FreeBytes>;

enum class StreamEnd { DONE, STOPPED, FAILED };   // STOPPED: the sink returned false; FAILED: errno says why (the reader's, or ENOMEM)

// Reads a stream to its end through `rd` (ssize_t(void*, size_t): read, gzread, ...) and hands it to `sink(Bytes&&, len, offset)` in
// batches cut EXACTLY where newline_cut cuts the whole stream, whatever sizes the reads return. For that a window is decided only
// once a byte behind it has been read, or the end of input is known: a stream that ends on a window goes out whole, as it does mapped.
// The rest behind a cut is carried into the next buffer. 16 spare bytes lie behind every buffer; an empty stream has no batch.
// read_batches_cut is the reader under a cut rule (CutBytes, CutUnits16); read_batches is the one of newline_cut, read_batches16 the one
// of newline_cut16.
template <class Read, class Sink, class Cut>
StreamEnd read_batches_cut(Read rd, size_t batch_bytes, Sink sink, Cut rule) {
    const size_t SPARE = 16, MAX_READ = (size_t)1 << 30;
    size_t cap = batch_bytes + 1, have = 0, searched = 0;   // searched != 0: no '\n' in buf[0, searched)
    uint64_t off = 0;
    bool eof = false;
    Bytes buf((uint8_t*)malloc(cap + SPARE));
    if (!buf) return StreamEnd::FAILED;
    for (;;) {
        size_t cut = 0;   // 0 = undecided: more bytes are needed
        if (eof) cut = rule.whole(buf.get(), have, batch_bytes);
        else if (have > batch_bytes) {
            cut = searched ? 0 : rule.last(buf.get(), batch_bytes);
            if (!cut) {   // a line longer than the window: to its end, looking at every byte once however the reads arrive
                if (searched < batch_bytes) searched = batch_bytes;
                cut = rule.first(buf.get(), searched, have);
                searched = have;
            }
        }
        if (!cut) {
            if (eof) return StreamEnd::DONE;
            if (have == cap) {   // a single line longer than the batch: grow
                uint8_t* nb = (uint8_t*)realloc(buf.get(), cap * 2 + SPARE);
                if (!nb) return StreamEnd::FAILED;
                buf.release(); buf.reset(nb); cap *= 2;
            }
            const ssize_t r = rd(buf.get() + have, cap - have < MAX_READ ? cap - have : MAX_READ);
            if (r < 0) { if (errno == EINTR) continue; return StreamEnd::FAILED; }
            if (r == 0) eof = true;
            have += (size_t)r;
            continue;
        }
        const size_t rest = have - cut;
        Bytes nxt;
        if (rest || !eof) {
            cap = rest > batch_bytes + 1 ? rest : batch_bytes + 1;
            nxt.reset((uint8_t*)malloc(cap + SPARE));
            if (!nxt) return StreamEnd::FAILED;
            memcpy(nxt.get(), buf.get() + cut, rest);
        }
        if (!sink(std::move(buf), cut, off)) return StreamEnd::STOPPED;
        if (!nxt) return StreamEnd::DONE;
        buf = std::move(nxt);
        off += cut; have = rest; searched = 0;
    }
}

template <class Read, class Sink>
StreamEnd read_batches(Read rd, size_t batch_bytes, Sink sink) { return read_batches_cut(rd, batch_bytes, sink, CutBytes{}); }
template <class Read, class Sink>
StreamEnd read_batches16(Read rd, size_t batch_bytes, uint32_t byte_order, Sink sink) { return read_batches_cut(rd, batch_bytes, sink, CutUnits16{byte_order}); }

// The whole pages inside [p, p + n): [a, b), true when there is one. Neighbouring batches never share a page of these ranges.
inline bool inner_pages(const void* p, size_t n, uintptr_t& a, uintptr_t& b) {
    const uintptr_t PAGE = 4096;
    a = ((uintptr_t)p + PAGE - 1) & ~(PAGE - 1);
    b = ((uintptr_t)p + n) & ~(PAGE - 1);
    return b > a;
}

// The READER faults a batch's pages in and pins its inner pages; the scanning threads only copy, scan and post-process. With every
// worker doing its own page faults and pinning, the address-space lock of the process was the limit (four workers: 28-31 GB/s; with
// the reader feeding them: 42-45). MATCHY_AMD_NO_FEEDER=1 restores that. Returns the pinned base (the batch's `pinned_range`, undone
// with matchy_amd_host_unregister) or null: small batches, no whole page, registration refused.
inline const void* prefault_and_pin(const uint8_t* p, size_t n) {
    static const bool feeder = getenv("MATCHY_AMD_NO_FEEDER") == nullptr;
    uintptr_t a, b;
    if (!feeder || n < ((size_t)4 << 20) || !inner_pages(p, n, a, b)) return nullptr;
#ifdef MADV_POPULATE_READ
    const uintptr_t lo = (uintptr_t)p & ~(uintptr_t)4095;
    (void)madvise((void*)lo, (uintptr_t)p + n - lo, MADV_POPULATE_READ);
#endif
    return matchy_amd_host_register((const void*)a, b - a) == MATCHY_SUCCESS ? (const void*)a : nullptr;
}

}  // namespace mxy
