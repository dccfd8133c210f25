// Harness of tests/test_gpu_extract_render_kernels.py: the kernels of csrc/extract_render.hip through their launch wrappers alone
// (csrc/extract_render.h), fed with candidate arrays made here, against a sequential host model built from csrc/extract_render_core.h.
//
// Every case runs in the three formats at the block capacities 0, d - 1, d, d + 1 and 2 d (d: the demand the model computes), the block
// inside an allocation with a poisoned guard band in front of it and behind it. One line per run:
//   CASE <name> fmt=F cap=C demand=D records=N short=S long=L <OK | FAIL: why>
// OK means: the demand the device counted is the model's; the counters (pairs, long list, records per type) are the model's; the bytes in
// front of min(demand, capacity) are the model's text; every byte at or behind it, and the guard in front, still holds the poison.
// The model asserts on its inputs that no two candidates share (rank, start) and does not rely on it (its sort is stable).
// The last line is DONE cases=<lines> failed=<FAIL lines>; the exit status is 0 when none failed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "extract_render.h"
#include "extract_render_core.h"
#include "line_index.h"

using namespace mxy;
namespace X = mxy::xrender;

#define CHECK(expr)                                                                                  \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) { printf("HIP ERROR %s: %s\n", #expr, hipGetErrorString(_e)); exit(3); } \
    } while (0)

static const Candidate PAD{0u, 0xFFFFFFFFu, 0u, 0u};
static Candidate cand(uint32_t start, uint32_t len, uint32_t type) { return Candidate{start, len | (type << 24), 0u, 0u}; }

struct Case {
    std::string name;
    std::vector<uint8_t> data;
    std::vector<Candidate> a, b;
};

struct Model { std::vector<uint8_t> text[X::FORMAT_COUNT]; uint32_t n = 0, n_long = 0; uint32_t by_type[IT_COUNT] = {0}; bool unique = true; };

static Model model_of(const Case& c) {
    Model m;
    struct Item { unsigned long long key; Candidate c; };
    std::vector<Item> items;
    std::set<std::pair<uint32_t, uint32_t>> seen;
    auto take = [&](const Candidate& e) {
        if (e.len_type == 0xFFFFFFFFu) return;
        uint32_t line = 0;
        for (uint32_t i = 0; i < e.start; ++i) line += c.data[i] == '\n';
        const uint32_t type = e.len_type >> 24;
        if (!seen.insert({X::rank(type), e.start}).second) m.unique = false;
        items.push_back(Item{X::key_pack(line, X::rank(type), e.start), e});
        if (type < IT_COUNT) m.by_type[type]++;
        if ((e.len_type & 0xFFFFFFu) > XR_SHORT_MAX) m.n_long++;
    };
    for (const Candidate& e : c.a) take(e);
    for (const Candidate& e : c.b) take(e);
    std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.key < y.key; });
    m.n = (uint32_t)items.size();
    for (uint32_t f = 0; f < X::FORMAT_COUNT; ++f) {
        uint64_t total = 0;
        for (const Item& it : items) {
            const uint32_t len = it.c.len_type & 0xFFFFFFu;
            total += X::record_len(f, it.c.len_type >> 24, len, X::count_escapes(f, c.data.data() + it.c.start, len));
        }
        m.text[f].resize(total);
        uint64_t pos = 0;
        for (const Item& it : items) pos += X::record_put(f, it.c.len_type >> 24, c.data.data() + it.c.start, it.c.len_type & 0xFFFFFFu, m.text[f].data(), pos, total);
    }
    return m;
}

template <class T> struct Dev {
    T* p = nullptr;
    explicit Dev(size_t n) { CHECK(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T))); }
    ~Dev() { (void)hipFree(p); }
};

static int g_lines = 0, g_failed = 0;
constexpr size_t GUARD = 4096;
constexpr uint8_t POISON = 0xA5;

static void run(const Case& c, const Model& m, uint32_t format, uint64_t cap) {
    const std::vector<uint8_t>& want = m.text[format];
    const uint32_t len = (uint32_t)c.data.size(), n = m.n, tiles = line_tiles(len);
    Dev<uint8_t> data(len);
    Dev<Candidate> la(c.a.size()), lb(c.b.size());
    if (len) CHECK(hipMemcpy(data.p, c.data.data(), len, hipMemcpyHostToDevice));
    if (!c.a.empty()) CHECK(hipMemcpy(la.p, c.a.data(), c.a.size() * sizeof(Candidate), hipMemcpyHostToDevice));
    if (!c.b.empty()) CHECK(hipMemcpy(lb.p, c.b.data(), c.b.size() * sizeof(Candidate), hipMemcpyHostToDevice));
    Dev<uint32_t> counts(tiles), chunks(line_chunks(tiles)), prefix(tiles + 1), vals(2 * (size_t)n), long_list(n);
    Dev<unsigned long long> keys(2 * (size_t)n);
    const size_t tb = sort_hits_temp_bytes(n);
    Dev<uint8_t> tmp(tb), block(GUARD + cap + GUARD);
    Dev<uint64_t> rec_len(n), rec_off((size_t)n + 1), sums(xr_chunks(n));
    Dev<XrCounters> ctr(1);
    CHECK(hipMemset(ctr.p, 0, sizeof(XrCounters)));
    CHECK(hipMemset(block.p, POISON, GUARD + cap + GUARD));
    XrInput in;
    in.data = data.p; in.len = len; in.list_a = la.p; in.n_a = (uint32_t)c.a.size(); in.list_b = lb.p; in.n_b = (uint32_t)c.b.size(); in.n_real = n; in.format = format;
    XrWork w{};
    w.line_counts = counts.p; w.line_chunks = chunks.p; w.line_prefix = prefix.p; w.keys = keys.p; w.vals = vals.p;
    w.sort_temp = tmp.p; w.sort_temp_bytes = tb; w.sort_half = xr_sort_half(tmp.p);
    w.rec_len = rec_len.p; w.rec_off = rec_off.p; w.chunk_sums = sums.p; w.long_list = long_list.p; w.ctr = ctr.p;
    CHECK(extract_render_order(in, w, 8, nullptr));
    CHECK(extract_render_measure(in, w, 8, nullptr));
    CHECK(extract_render_write(in, w, block.p + GUARD, cap, 8, nullptr));
    CHECK(hipDeviceSynchronize());
    XrCounters h;
    CHECK(hipMemcpy(&h, ctr.p, sizeof(h), hipMemcpyDeviceToHost));
    std::vector<uint8_t> got(GUARD + cap + GUARD);
    CHECK(hipMemcpy(got.data(), block.p, got.size(), hipMemcpyDeviceToHost));

    std::string why;
    if (!m.unique) why = "the case has two candidates with one (rank, start)";
    else if (h.out.status != XR_OK) why = "status " + std::to_string(h.out.status);
    else if (h.pairs.n_pairs != n) why = "pairs " + std::to_string(h.pairs.n_pairs);
    else if (h.longs.n_long != m.n_long) why = "long list " + std::to_string(h.longs.n_long) + " want " + std::to_string(m.n_long);
    else if (h.out.demand != want.size()) why = "demand " + std::to_string(h.out.demand) + " want " + std::to_string(want.size());
    for (int t = 0; t < IT_COUNT && why.empty(); ++t)
        if (h.by_type[t].n != m.by_type[t]) why = "type " + std::to_string(t) + " counted " + std::to_string(h.by_type[t].n) + " want " + std::to_string(m.by_type[t]);
    if (why.empty()) {
        const uint64_t end = std::min<uint64_t>(want.size(), cap);
        for (size_t k = 0; k < GUARD && why.empty(); ++k) if (got[k] != POISON) why = "a byte in front of the block";
        for (uint64_t k = 0; k < end && why.empty(); ++k)
            if (got[GUARD + k] != want[k]) why = "byte " + std::to_string(k) + " is " + std::to_string(got[GUARD + k]) + " want " + std::to_string(want[k]);
        for (uint64_t k = end; k < cap + GUARD && why.empty(); ++k) if (got[GUARD + k] != POISON) why = "a byte at or behind min(demand, capacity): " + std::to_string(k);
    }
    ++g_lines;
    if (!why.empty()) ++g_failed;
    printf("CASE %s fmt=%u cap=%llu demand=%llu records=%u short=%u long=%u %s\n", c.name.c_str(), format, (unsigned long long)cap,
           (unsigned long long)h.out.demand, h.pairs.n_pairs, h.pairs.n_pairs - std::min(h.longs.n_long, h.pairs.n_pairs), h.longs.n_long,
           why.empty() ? "OK" : ("FAIL: " + why).c_str());
    fflush(stdout);
}

// ------------------------------------------------------------------------------------------------ cases
static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
template <class T> static void shuffle(std::vector<T>& v) { for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[rnd() % i]); }

// splits `all` over the two lists and puts runs of padding at the head, the middle and the end of both
static void split_with_padding(Case& c, std::vector<Candidate> all, bool pad) {
    shuffle(all);
    const size_t half = all.size() / 2;
    auto fill = [&](std::vector<Candidate>& l, size_t from, size_t to) {
        if (pad) l.insert(l.end(), 3, PAD);
        for (size_t i = from; i < to; ++i) {
            l.push_back(all[i]);
            if (pad && i == (from + to) / 2) l.insert(l.end(), 70, PAD);   // more than a wave of padding
        }
        if (pad) l.insert(l.end(), 5, PAD);
    };
    fill(c.a, 0, half);
    fill(c.b, half, all.size());
}

// n candidates of 3 .. 6 bytes, a line end behind every `per_line`-th, the types in rotation
static Case many(const std::string& name, uint32_t n, uint32_t per_line, bool pad) {
    Case c;
    c.name = name;
    std::vector<Candidate> all;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = 3 + i % 4, start = (uint32_t)c.data.size();
        for (uint32_t k = 0; k < len; ++k) c.data.push_back((uint8_t)("abc\"d\\ef"[(i + k) % 8]));
        all.push_back(cand(start, len, i % IT_COUNT));
        c.data.push_back((i + 1) % per_line == 0 ? '\n' : ' ');
    }
    split_with_padding(c, all, pad);
    return c;
}

static std::vector<Case> cases() {
    std::vector<Case> v;
    { Case c; c.name = "zero_entries"; c.data.assign({'a', '\n', 'b'}); v.push_back(c); }
    { Case c; c.name = "padding_only"; c.data.assign(100, 'x'); c.a.assign(130, PAD); c.b.assign(7, PAD); v.push_back(c); }
    { Case c; c.name = "one_candidate"; const char* s = "first\nsecond 10.1.2.3 x\n"; c.data.assign(s, s + strlen(s)); c.b.push_back(cand(13, 8, IT_IPV4)); v.push_back(c); }
    v.push_back(many("two_lists_padding", 300, 4, true));
    v.push_back(many("n2047", 2047, 3, false));
    v.push_back(many("n2048", 2048, 5, true));
    v.push_back(many("n2049", 2049, 1, false));
    v.push_back(many("n4097", 4097, 2, true));
    {   // one line with one candidate of each rank, listed from the last rank to the first; a second line in front of it in the list
        Case c; c.name = "eight_ranks_reverse";
        const uint32_t type_of_rank[8] = {IT_DOMAIN, IT_IPV4, IT_EMAIL, IT_IPV6, IT_SHA256, IT_BITCOIN, IT_ETHEREUM, IT_MONERO};
        const char* s = "zero\nr0 r1 r2 r3 r4 r5 r6 r7\nlast";
        c.data.assign(s, s + strlen(s));
        c.a.push_back(cand(29, 4, IT_DOMAIN));
        for (int r = 7; r >= 0; --r) c.a.push_back(cand(5 + 3 * (uint32_t)r, 2, type_of_rank[r]));
        c.a.push_back(cand(0, 4, IT_MD5));
        v.push_back(c);
    }
    {   // lines whose '\n' sit at offsets 1023, 1024 and 1025 of a tile, candidates on both sides of each and across the tile edges
        Case c; c.name = "newline_tile_edges";
        c.data.assign(6 * 1024, 'k');
        const uint32_t nl[] = {1023, 1024 + 1024, 2 * 1024 + 1025, 4 * 1024 + 1023};   // the last byte of a tile, the first and the second of the next
        for (uint32_t p : nl) c.data[p] = '\n';
        std::vector<Candidate> all;
        for (uint32_t p : nl) {
            all.push_back(cand(p - 3, 3, IT_DOMAIN));    // ends at the '\n'
            all.push_back(cand(p + 1, 2, IT_EMAIL));     // begins behind it
            all.push_back(cand(p - 40, 20, IT_SHA1));
        }
        for (uint32_t t = 1; t < 6; ++t) all.push_back(cand(t * 1024 - 17, 9, IT_MONERO));
        all.push_back(cand(0, 1, IT_IPV6));
        split_with_padding(c, all, true);
        v.push_back(c);
    }
    { Case c = many("no_newline", 200, 1000000, true); v.push_back(c); }
    {   // the batch ends in the last byte of a candidate (no line end, no byte behind it)
        Case c; c.name = "ends_in_candidate";
        const char* s = "a.example.org\nb\"c\\";
        c.data.assign(s, s + strlen(s));
        c.a.push_back(cand((uint32_t)strlen(s) - 4, 4, IT_EMAIL));
        c.a.push_back(cand(0, 13, IT_DOMAIN));
        v.push_back(c);
    }
    {   // escapes at every alignment of the start and every position of texts of 1 .. 9 bytes
        Case c; c.name = "escape_alignments";
        std::vector<Candidate> all;
        for (uint32_t len = 1; len <= 9; ++len)
            for (uint32_t at = 0; at < len; ++at)
                for (uint32_t align = 0; align < 4; ++align) {
                    while (c.data.size() % 4 != align) c.data.push_back('.');
                    const uint32_t start = (uint32_t)c.data.size();
                    for (uint32_t k = 0; k < len; ++k) c.data.push_back(k == at ? ((len + at) & 1 ? '"' : '\\') : (k == at + 1 ? '"' : 'm'));
                    all.push_back(cand(start, len, (len + at + align) % IT_COUNT));
                    c.data.push_back(start % 7 == 0 ? '\n' : ' ');
                }
        split_with_padding(c, all, false);
        v.push_back(c);
    }
    {   // both tiers: 512 is the last length a lane takes; the long ones cross many strides of a wave, with escapes in them
        Case c; c.name = "long_candidates";
        std::vector<Candidate> all;
        const uint32_t lens[] = {100000, 512, 4099, 513, 7};
        uint32_t type = 0;
        for (uint32_t len : lens) {
            const uint32_t start = (uint32_t)c.data.size();
            for (uint32_t k = 0; k < len; ++k) c.data.push_back(k % 61 == 0 ? '"' : k % 97 == 3 ? '\\' : (uint8_t)('a' + k % 26));
            c.data[start + len - 1] = '"';
            all.push_back(cand(start, len, type++ % IT_COUNT));
            c.data.push_back(type % 2 ? '\n' : ' ');
        }
        split_with_padding(c, all, true);
        v.push_back(c);
    }
    {   // keys equal in line and rank that differ only in start: the five hash types share a rank
        Case c; c.name = "same_line_and_rank";
        c.data.assign(4000, 'h');
        c.data[2000] = '\n';
        std::vector<Candidate> all;
        for (uint32_t i = 0; i < 300; ++i) all.push_back(cand(i * 13 + (i >= 150 ? 60 : 0), 11, IT_MD5 + i % 5));
        split_with_padding(c, all, true);
        v.push_back(c);
    }
    return v;
}

int main() {
    for (const Case& c : cases()) {
        const Model m = model_of(c);
        for (uint32_t f = 0; f < X::FORMAT_COUNT; ++f) {
            const uint64_t d = m.text[f].size();
            std::vector<uint64_t> caps;
            if (d == 0) caps = {0, 1}; else caps = {0, d - 1, d, d + 1, 2 * d};
            for (uint64_t cap : caps) run(c, m, f, cap);
        }
    }
    printf("DONE cases=%d failed=%d\n", g_lines, g_failed);
    return g_failed ? 1 : 0;
}
