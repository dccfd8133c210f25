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

// malloc'ed bytes (no value-initialisation: a 256 MiB batch buffer would be zeroed before every read; realloc grows it for a long
// line). Whoever takes a batch from the reader owns it; across the C ABI it travels as release() and comes back through free().
struct FreeBytes { void operator()(uint8_t* p) const { free(p); } };
using Bytes = std::unique_ptr<uint8_t[], FreeBytes>;

enum class StreamEnd { DONE, STOPPED, FAILED };   // STOPPED: the sink returned false; FAILED: errno says why (the reader's, or ENOMEM)

// Reads a stream to its end through `rd` (ssize_t(void*, size_t): read, gzread, ...) and hands it to `sink(Bytes&&, len, offset)` in
// batches cut EXACTLY where newline_cut cuts the whole stream, whatever sizes the reads return. For that a window is decided only
// once a byte behind it has been read, or the end of input is known: a stream that ends on a window goes out whole, as it does mapped.
// The rest behind a cut is carried into the next buffer. 16 spare bytes lie behind every buffer; an empty stream has no batch.
template <class Read, class Sink>
StreamEnd read_batches(Read rd, size_t batch_bytes, Sink sink) {
    const size_t SPARE = 16, MAX_READ = (size_t)1 << 30;
    size_t cap = batch_bytes + 1, have = 0, searched = 0;   // searched != 0: no '\n' in buf[0, searched)
    uint64_t off = 0;
    bool eof = false;
    Bytes buf((uint8_t*)malloc(cap + SPARE));
    if (!buf) return StreamEnd::FAILED;
    for (;;) {
        size_t cut = 0;   // 0 = undecided: more bytes are needed
        if (eof) cut = newline_cut(buf.get(), 0, have, batch_bytes);
        else if (have > batch_bytes) {
            const void* nl = searched ? nullptr : memrchr(buf.get(), '\n', batch_bytes);
            if (!nl) {   // a line longer than the window: to its end, looking at every byte once however the reads arrive
                if (searched < batch_bytes) searched = batch_bytes;
                nl = memchr(buf.get() + searched, '\n', have - searched);
                searched = have;
            }
            if (nl) cut = (size_t)((const uint8_t*)nl - buf.get()) + 1;
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
