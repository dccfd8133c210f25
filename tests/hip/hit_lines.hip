// GPU: the launch wrappers of csrc/hit_lines.h against a sequential host model (driver: tests/test_gpu_hit_lines_kernels.py).
//
// A case is a batch of lines, some of which "hit": every hit line gets one or more line records (as k_line_resolve would write them,
// here computed on the host), shuffled and split into the 16-byte-record array and the compact one. The model is the block contract of
// include/matchy_amd.h, written from that text: the distinct hit lines in ascending order, each ended by '\n'.
//
// The batch is uploaded into an allocation of exactly its length. The block is allocated as GUARD + max(capacity, demand) + GUARD bytes
// and filled with a poison byte that no batch contains: a store that misses its bound lands inside the allocation, where the host finds
// it, and never faults. The whole chain (mark, rank, lengths, offsets, copy) runs once per capacity: 0, demand - 1, demand, demand + 1
// and 2 x demand.
//
// Checked for every (case, capacity):
//   1. n_lines and text_len (the demand) equal the model's, whatever the capacity
//   2. line_off[0 .. n_lines], line_no and line_of equal the model's
//   3. both guard bands and every byte at or behind min(demand, capacity) still hold poison
//   4. the bytes in front of min(demand, capacity) equal the model's block (all of it when the demand fits)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "hit_lines.h"

using namespace mxy;

constexpr uint32_t GUARD = 8192;       // a multiple of 16: the block behind it is 16-byte aligned
constexpr uint8_t POISON = 0xA5;       // the batches are ASCII
constexpr int N_CU = 8;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FATAL %s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(3); } } while (0)

struct Case {
    std::string name;
    std::string batch;
    std::vector<uint32_t> hit_lines;   // line numbers, with repeats: one record each
};

// appends a line of `len` bytes (no '\n' inside) and, if terminated, its '\n'; returns its number
struct Builder {
    std::string b;
    uint32_t n = 0;
    std::mt19937 rng{12345};
    uint32_t line(uint32_t len, bool terminated = true) {
        for (uint32_t k = 0; k < len; ++k) b.push_back((char)('a' + rng() % 26));
        if (terminated) b.push_back('\n');
        return n++;
    }
    // a filler line (never a hit) so that the next line starts at residue r mod 16
    void pad_to(uint32_t r) { line((r + 16u - (uint32_t)((b.size() + 1) % 16)) % 16u); }
};

struct Model {
    std::vector<LineRec> recs;          // per record
    std::vector<uint32_t> line_off, line_no, line_of;
    std::string text;
};

static Model model_of(const Case& c, uint32_t& n_newlines) {
    std::vector<uint32_t> starts{0};
    for (size_t i = 0; i < c.batch.size(); ++i) if (c.batch[i] == '\n') starts.push_back((uint32_t)i + 1);
    n_newlines = (uint32_t)starts.size() - 1;
    auto end_of = [&](uint32_t l) { return l + 1 < starts.size() ? starts[l + 1] - 1 : (uint32_t)c.batch.size(); };
    Model m;
    std::map<uint32_t, uint32_t> rank;
    for (uint32_t l : c.hit_lines) rank[l] = 0;
    m.line_off.push_back(0);
    for (auto& kv : rank) {
        kv.second = (uint32_t)m.line_no.size();
        m.line_no.push_back(kv.first);
        m.text.append(c.batch, starts[kv.first], end_of(kv.first) - starts[kv.first]);
        m.text.push_back('\n');
        m.line_off.push_back((uint32_t)m.text.size());
    }
    for (uint32_t l : c.hit_lines) { m.recs.push_back(LineRec{l, starts[l], end_of(l), 0}); m.line_of.push_back(rank[l]); }
    return m;
}

static std::vector<Case> cases() {
    std::vector<Case> out;
    std::mt19937 rng(777);
    auto shuffled = [&](Case c) { std::shuffle(c.hit_lines.begin(), c.hit_lines.end(), rng); return c; };
    {   // every start residue mod 16 x lengths 0..40; the first line of the batch (offset 0) hits; one line carries 200 records
        Case c{"residues", "", {}};
        Builder b;
        c.hit_lines.push_back(b.line(7));
        for (uint32_t r = 0; r < 16; ++r)
            for (uint32_t len = 0; len <= 40; ++len) { b.pad_to(r); c.hit_lines.push_back(b.line(len)); }
        for (int k = 0; k < 199; ++k) c.hit_lines.push_back(c.hit_lines[100]);
        c.batch = b.b;
        out.push_back(shuffled(c));
    }
    for (int d = -1; d <= 1; ++d) {   // a line whose terminator is the last byte of a slice, the one before it, the first of the next
        Case c{std::string("slice_edge") + (d < 0 ? "-1" : d == 0 ? "+0" : "+1"), "", {}};
        Builder b;
        b.line(3);
        c.hit_lines.push_back(b.line(HIT_LINES_SLICE - 1 + d));
        for (int k = 0; k < 300; ++k) { const uint32_t l = b.line(20); if (k % 3 != 1) c.hit_lines.push_back(l); }
        c.hit_lines.push_back(b.line(2 * HIT_LINES_SLICE - 6001 - d));   // ends the second slice's neighbourhood at another residue
        c.hit_lines.push_back(b.line(33));
        c.batch = b.b;
        out.push_back(shuffled(c));
    }
    {   // one line of 3 slices + 5 bytes between short ones
        Case c{"long_line", "", {}};
        Builder b;
        b.line(5);
        c.hit_lines.push_back(b.line(12));
        c.hit_lines.push_back(b.line(3 * HIT_LINES_SLICE + 5));
        c.hit_lines.push_back(b.line(12));
        c.batch = b.b;
        out.push_back(shuffled(c));
    }
    for (uint32_t tail : {1u, 15u, 16u, 17u, 100u, 5000u}) {   // an unterminated last line: its last byte is the last byte of the allocation
        Case c{"unterminated" + std::to_string(tail), "", {}};
        Builder b;
        c.hit_lines.push_back(b.line(9));
        b.line(4);
        c.hit_lines.push_back(b.line(tail, false));
        c.batch = b.b;
        out.push_back(shuffled(c));
    }
    {   // more words than one workgroup of the rank step covers and more hit lines than one workgroup of the offset step covers;
        // hit lines on both sides of the chunk boundary (line 32 * HIT_LINES_SCAN_CHUNK) and of word boundaries
        Case c{"many_lines", "", {}};
        Builder b;
        const uint32_t edge = 32u * HIT_LINES_SCAN_CHUNK;
        for (uint32_t l = 0; l < edge + 5000; ++l) {
            const bool hit = l % 13 == 0 || l == 31 || l == 32 || l == 63 || l == 64 || l == edge - 1 || l == edge || l == edge + 1;
            b.line(hit ? 1 + l % 7 : 0);
            if (hit) c.hit_lines.push_back(l);
        }
        c.batch = b.b;
        out.push_back(shuffled(c));
    }
    {   // no record at all
        Case c{"empty", "abc\ndef\n", {}};
        out.push_back(c);
    }
    return out;
}

template <class T> struct Dev {
    T* p = nullptr;
    explicit Dev(size_t n) { HIP_OK(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T))); }
    ~Dev() { (void)hipFree(p); }
};

static std::string run_case(const Case& c, const Model& m, uint32_t n_newlines, uint32_t capacity, uint32_t& demand_out) {
    const uint32_t n = (uint32_t)m.recs.size(), n_fin = n - n / 3, n_c4 = n - n_fin;   // the last third plays the compact records
    const uint64_t n_bits = (uint64_t)n_newlines + 1;
    const uint32_t words = hit_line_words(n_bits), demand = (uint32_t)m.text.size();
    Dev<uint8_t> data(c.batch.size());   // exactly the batch: a load behind it leaves the allocation
    Dev<LineRec> recs(n);
    Dev<uint32_t> bitmap(words), word_prefix(words + 1), chunks(std::max(hit_line_chunks(words), hit_line_chunks(n)));
    Dev<uint32_t> src(n), len(n), line_no(n), line_of(n), line_off(n + 1);
    Dev<HitLineCounters> ctr(1);
    const size_t room = (size_t)GUARD + std::max(capacity, demand) + GUARD;
    Dev<uint8_t> block(room);
    HIP_OK(hipMemcpy(data.p, c.batch.data(), c.batch.size(), hipMemcpyHostToDevice));
    if (n) HIP_OK(hipMemcpy(recs.p, m.recs.data(), n * sizeof(LineRec), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(block.p, POISON, room));
    HIP_OK(hipMemset(ctr.p, 0, sizeof(HitLineCounters)));
    HIP_OK(hipMemset(bitmap.p, 0, (size_t)words * 4));
    HIP_OK(hipMemset(line_off.p, 0xFF, ((size_t)n + 1) * 4));
    HIP_OK(hit_lines_mark_rank(recs.p, n_fin, recs.p + n_fin, n_c4, bitmap.p, n_bits, chunks.p, word_prefix.p, ctr.p, nullptr));
    HIP_OK(hit_lines_offsets(recs.p, n_fin, recs.p + n_fin, n_c4, bitmap.p, n_bits, word_prefix.p, src.p, len.p, line_no.p, line_of.p, chunks.p, line_off.p, ctr.p,
                             nullptr));
    HIP_OK(hit_lines_copy(data.p, (uint32_t)c.batch.size(), ctr.p, src.p, line_off.p, block.p + GUARD, capacity, N_CU, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HitLineCounters hc;
    HIP_OK(hipMemcpy(&hc, ctr.p, sizeof(hc), hipMemcpyDeviceToHost));
    demand_out = hc.text_len;
    char msg[256];
    if (hc.n_lines != m.line_no.size() || hc.text_len != demand) {
        snprintf(msg, sizeof msg, "counters n_lines=%u text_len=%u, model %zu %u", hc.n_lines, hc.text_len, m.line_no.size(), demand);
        return msg;
    }
    std::vector<uint32_t> got_off(n + 1), got_no(n), got_of(n);
    HIP_OK(hipMemcpy(got_off.data(), line_off.p, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost));
    if (n) {
        HIP_OK(hipMemcpy(got_no.data(), line_no.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_of.data(), line_of.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    }
    for (size_t k = 0; k < m.line_off.size(); ++k)
        if (got_off[k] != m.line_off[k]) { snprintf(msg, sizeof msg, "line_off[%zu]=%u, model %u", k, got_off[k], m.line_off[k]); return msg; }
    for (size_t k = 0; k < m.line_no.size(); ++k)
        if (got_no[k] != m.line_no[k]) { snprintf(msg, sizeof msg, "line_no[%zu]=%u, model %u", k, got_no[k], m.line_no[k]); return msg; }
    for (size_t i = 0; i < n; ++i)
        if (got_of[i] != m.line_of[i]) { snprintf(msg, sizeof msg, "line_of[%zu]=%u, model %u", i, got_of[i], m.line_of[i]); return msg; }
    std::vector<uint8_t> got(room);
    HIP_OK(hipMemcpy(got.data(), block.p, room, hipMemcpyDeviceToHost));
    const uint32_t written = std::min(demand, capacity);
    for (size_t k = 0; k < room; ++k) {
        const bool inside = k >= GUARD && k < (size_t)GUARD + written;
        const uint8_t want = inside ? (uint8_t)m.text[k - GUARD] : POISON;
        if (got[k] != want) {
            snprintf(msg, sizeof msg, "block byte %lld is 0x%02x, expected 0x%02x (%s)", (long long)k - (long long)GUARD, got[k], want, inside ? "content" : "poison");
            return msg;
        }
    }
    return "";
}

int main() {
    int n_cases = 0, failed = 0;
    for (const Case& c : cases()) {
        uint32_t n_newlines = 0;
        const Model m = model_of(c, n_newlines);
        const uint32_t demand = (uint32_t)m.text.size();
        std::vector<uint32_t> caps{0u, demand ? demand - 1 : 0u, demand, demand + 1, 2 * demand};
        if (!demand) caps = {0u, 1u};
        for (uint32_t cap : caps) {
            uint32_t got_demand = 0;
            const std::string verdict = run_case(c, m, n_newlines, cap, got_demand);
            printf("CASE %s cap=%u demand=%u lines=%zu records=%zu %s\n", c.name.c_str(), cap, got_demand, m.line_no.size(), m.recs.size(),
                   verdict.empty() ? "OK" : ("FAIL: " + verdict).c_str());
            fflush(stdout);
            ++n_cases;
            if (!verdict.empty()) ++failed;
        }
    }
    printf("DONE cases=%d failed=%d\n", n_cases, failed);
    return failed ? 1 : 0;
}
