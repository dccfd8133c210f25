// GPU: the launch wrappers of csrc/render.h against a sequential host model built from csrc/render_core.h (driver:
// tests/test_gpu_render_kernels.py).
//
// A case is a batch, hit records over it (16-byte records, then compact IPv4 ones), the data offsets of the pattern ids, a payload
// text per data offset, sources and line bases (one, or one per segment) and the render flags. Line records, segment indices and the
// '\n' count in front of each segment are computed here on the host, as the passes in front of the renderer would leave them. The
// model walks the records in order through render::record_emit with the sequential sinks.
//
// The batch is uploaded into an allocation of exactly its length. The block is allocated as GUARD + max(capacity, demand) + GUARD bytes
// and filled with a poison byte that no case contains; the miss list has a poisoned guard behind its capacity. A store that misses its
// bound lands inside the allocation, where the host finds it, and never faults.
//
// Per case:
//   MISS   the payload table empty, at miss-list capacities 0, misses - 1 and misses: the count equals the distinct data offsets of the
//          case whatever the capacity, the entries in front of the capacity are distinct offsets of the case, the guard holds poison
//   CASE   the table filled, at block capacities 0, demand - 1, demand, demand + 1 and 2 x demand: no miss, the demand equals the
//          model's, both guard bands and every byte at or behind min(demand, capacity) hold poison, the bytes in front equal the model's
//   CROWDED the table empty and a miss set of two slots: the list may repeat offsets, holds every offset of the case and nothing else
//   PIECES (cases with long records) piece arrays one slot too small: the pass says so, counts the slots it needs, stores nothing
//   SWEEP  every capacity within 40 bytes of record boundaries — those where a wave's run of short records begins (records 64, 128,
//          2048, the record behind a long one) among them: the same checks as CASE
//   LIMIT  a byte limit below the demand: RENDER_TOO_LARGE, the demand still counted, nothing stored
// The CASE runs alternate between the grids the long list gets with and without a hint of long records from the scan before.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "render.h"
#include "render_core.h"

using namespace mxy;
namespace R = mxy::render;

constexpr uint32_t GUARD = 8192;
constexpr uint8_t POISON = 0xA5;   // no batch, payload or source holds it
constexpr uint32_t LIST_GUARD = 64;
constexpr int N_CU = 8;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FATAL %s: %s\n", #x, hipGetErrorString(e_)); fflush(stdout); exit(3); } } while (0)

struct HostRec { uint32_t start, len, value; uint8_t kind, prefix; uint16_t n_ids; };

struct Case {
    std::string name;
    std::string batch;
    std::vector<HostRec> fin, c4;                 // c4: IPv4 results that travel in the compact form
    std::vector<int64_t> data_offsets;
    std::map<uint32_t, std::string> payloads;     // every data offset the records name
    uint32_t flags = R::FLAG_LINE_NUMBERS | R::FLAG_INPUT_LINE;
    std::vector<uint32_t> seg_starts;             // empty: no segments
    std::vector<std::string> sources{"-"};        // raw; one, or one per segment
    std::vector<uint64_t> line_bases{0};
};

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n = 0;
    explicit Dev(size_t count) : n(count) { HIP_OK(hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T))); }
    explicit Dev(const std::vector<T>& v) : Dev(v.size()) { if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice)); }
    ~Dev() { (void)hipFree(p); }
    Dev(const Dev&) = delete;
    std::vector<T> host() const { std::vector<T> v(n); if (n) HIP_OK(hipMemcpy(v.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); return v; }
    void fill(int byte) { HIP_OK(hipMemset(p, byte, std::max<size_t>(n, 1) * sizeof(T))); }
};

static std::string escaped(const std::string& s) {   // json_escape with its quotes, through the rules under test's sequential form
    R::LenSink ls;
    ls.text(reinterpret_cast<const uint8_t*>(s.data()), (uint32_t)s.size());
    std::string o(ls.n + 2, '"');
    R::PutSink ps{reinterpret_cast<uint8_t*>(&o[1]), 0, ls.n};
    ps.text(reinterpret_cast<const uint8_t*>(s.data()), (uint32_t)s.size());
    return o;
}

// ------------------------------------------------------------------------------------------------ the model
struct ModelPayloads {
    const Case& c;
    template <class S> void one(S& s, uint32_t off) { const std::string& j = c.payloads.at(off); s.bytes(reinterpret_cast<const uint8_t*>(j.data()), (uint32_t)j.size()); }
    template <class S> void array(S& s, uint32_t first, uint32_t n) {
        bool any = false;
        for (uint32_t k = 0; k < n; ++k) {
            const int64_t d = c.data_offsets[first + k];
            if (d < 0) continue;
            if (any) MXY_RC_LIT(s, ","); else MXY_RC_LIT(s, "\"data\":[");
            one(s, (uint32_t)d);
            any = true;
        }
        if (any) MXY_RC_LIT(s, "],");
    }
};

struct Model {
    std::vector<LineRec> fin_lines, c4_lines;
    std::vector<uint32_t> seg_of_fin, seg_of_c4, seg_line_base;
    std::vector<RenderSource> sources;
    std::string source_text, text;
    std::set<uint32_t> offsets;   // distinct data offsets
    uint32_t n_short = 0, n_long = 0, n_pieces = 0;
};

static Model model_of(const Case& c) {
    Model m;
    std::vector<uint32_t> starts{0};
    for (size_t i = 0; i < c.batch.size(); ++i) if (c.batch[i] == '\n') starts.push_back((uint32_t)i + 1);
    auto line_of = [&](uint32_t at) {
        const uint32_t l = (uint32_t)(std::upper_bound(starts.begin(), starts.end(), at) - starts.begin()) - 1;
        const uint32_t end = l + 1 < starts.size() ? starts[l + 1] - 1 : (uint32_t)c.batch.size();
        return LineRec{l, starts[l], end, 0};
    };
    for (const std::string& s : c.sources) { const std::string e = escaped(s); m.sources.push_back(RenderSource{(uint32_t)m.source_text.size(), (uint32_t)e.size()}); m.source_text += e; }
    for (uint32_t st : c.seg_starts) m.seg_line_base.push_back((uint32_t)std::count(c.batch.begin(), c.batch.begin() + st, '\n'));
    const uint8_t* data = reinterpret_cast<const uint8_t*>(c.batch.data());
    ModelPayloads pay{c};
    R::LenSink total;
    std::vector<uint8_t> out;
    for (int pass = 0; pass < 2; ++pass) {   // measure everything, then write into a block of exactly that length
        R::PutSink put{out.data(), 0, out.size()};
        for (size_t i = 0; i < c.fin.size() + c.c4.size(); ++i) {
            const bool in_fin = i < c.fin.size();
            const HostRec& h = in_fin ? c.fin[i] : c.c4[i - c.fin.size()];
            const LineRec lr = line_of(h.start);
            uint32_t seg = 0;
            if (!c.seg_starts.empty()) seg = (uint32_t)(std::upper_bound(c.seg_starts.begin(), c.seg_starts.end(), h.start) - c.seg_starts.begin()) - 1;
            R::RecordIn r{};
            r.hit = data + h.start; r.hit_len = h.len; r.value = h.value; r.n_ids = h.kind == 2 ? 0 : h.n_ids; r.kind = h.kind; r.prefix_len = h.prefix;
            r.flags = c.flags;
            r.line = data + lr.line_start; r.line_len = lr.line_end - lr.line_start;
            r.line_number = c.line_bases[seg] + (lr.line - (c.seg_starts.empty() ? 0 : m.seg_line_base[seg])) + 1;
            r.source = reinterpret_cast<const uint8_t*>(m.source_text.data()) + m.sources[seg].off; r.source_len = m.sources[seg].len;
            if (pass == 0) {
                (in_fin ? m.fin_lines : m.c4_lines).push_back(lr);
                (in_fin ? m.seg_of_fin : m.seg_of_c4).push_back(seg);
                if (h.kind == 2) m.offsets.insert(h.value);
                else for (uint32_t k = 0; k < h.n_ids; ++k) if (c.data_offsets[h.value + k] >= 0) m.offsets.insert((uint32_t)c.data_offsets[h.value + k]);
                const uint32_t line_bytes = (c.flags & R::FLAG_INPUT_LINE) ? r.line_len : 0;
                const uint64_t before = total.n;
                R::record_emit(r, pay, total);
                if ((uint64_t)h.len + line_bytes <= RENDER_SHORT_MAX && r.n_ids <= RENDER_SHORT_IDS && total.n - before <= RENDER_SHORT_TEXT) ++m.n_short;
                else { ++m.n_long; m.n_pieces += render_pieces(h.len) + ((c.flags & R::FLAG_INPUT_LINE) ? render_pieces(r.line_len) : 0); }
            } else R::record_emit(r, pay, put);
        }
        if (pass == 0) out.resize(total.n);
        else if (put.pos != total.n) { printf("FATAL the model wrote %llu of %llu bytes\n", (unsigned long long)put.pos, (unsigned long long)total.n); exit(3); }
    }
    m.text.assign(out.begin(), out.end());
    return m;
}

// ------------------------------------------------------------------------------------------------ cases
struct Builder {
    Case c;
    uint32_t next_value = 0x100;
    explicit Builder(const std::string& name) { c.name = name; }
    uint32_t at() const { return (uint32_t)c.batch.size(); }
    void raw(const std::string& s) { c.batch += s; }
    std::string letters(uint32_t n, uint32_t seed = 0) { std::string s; for (uint32_t k = 0; k < n; ++k) s.push_back((k + seed) % 11 == 10 ? ' ' : (char)('a' + (k * 7 + seed) % 26)); return s; }
    uint32_t payload(const std::string& json) { const uint32_t v = next_value; next_value += 24; c.payloads[v] = json; return v; }
    // a pattern record over [start, start + len) with n ids; has(k): id k carries data
    template <class F>
    void pattern(uint32_t start, uint32_t len, uint32_t n, F has) {
        const uint32_t first = (uint32_t)c.data_offsets.size();
        for (uint32_t k = 0; k < n; ++k) c.data_offsets.push_back(has(k) ? (int64_t)payload("{\"id\":" + std::to_string(first + k) + ",\"t\":\"x\\\"y\"}") : -1);
        c.fin.push_back(HostRec{start, len, first, 3, 0, (uint16_t)n});
    }
    void ip(uint32_t start, uint32_t len, uint8_t prefix, bool compact = false) {
        const uint32_t v = payload("{\"net\":" + std::to_string(c.fin.size() + c.c4.size()) + "}");
        (compact ? c.c4 : c.fin).push_back(HostRec{start, len, v, 2, prefix, 0});
    }
    // a line "<lead> <token> <tail>\n"; returns the offset of the token
    uint32_t line_with(const std::string& token, uint32_t lead, uint32_t tail, bool terminated = true) {
        raw(letters(lead, at()) + " ");
        const uint32_t t = at();
        raw(token + " " + letters(tail, at()));
        if (terminated) raw("\n");
        return t;
    }
};
static bool always(uint32_t) { return true; }
static bool never(uint32_t) { return false; }

static std::vector<Case> cases() {
    std::vector<Case> out;
    {   // hit + line = RENDER_SHORT_MAX - 1 / + 0 / + 1 source bytes; 8 and 9 ids
        Builder b("tier_edges");
        for (int d = -1; d <= 1; ++d) {   // token of 10 bytes in a line of RENDER_SHORT_MAX + d - 10 bytes
            const uint32_t line_len = RENDER_SHORT_MAX + d - 10, lead = 40, tail = line_len - lead - 1 - 10 - 1;
            b.pattern(b.line_with("tok\"en\\.10", lead, tail), 10, 2, always);
        }
        b.pattern(b.line_with("eight.ids", 5, 5), 9, 8, always);
        b.pattern(b.line_with("nine.ids", 5, 5), 8, 9, always);
        out.push_back(b.c);
    }
    {   // one line of 3 x RENDER_PIECE + 1 bytes with two hits; ill-formed UTF-8 and escapes at -3 .. +3 around every piece edge
        Builder b("long_line");
        b.line_with("10.1.2.3", 3, 3);
        const uint32_t P = RENDER_PIECE;
        const char e1[7] = {(char)0xF0, (char)0x90, (char)0x80, (char)0x80, '"', '\t', (char)0xFF};        // a 4-byte sequence
        const char e2[7] = {0x5C, (char)0xE0, (char)0xA0, 'A', (char)0x80, 0x01, '"'};                      // a 3-byte sequence cut short by 'A'
        const char e3[4] = {0x1F, (char)0xC2, (char)0xA9, (char)0xE2};                                        // a lead byte as the line's last byte
        // seven such lines: the patterns shifted by -3 .. +3 against the piece edges, so that every byte of them meets an edge from
        // both sides (the last pattern ends the line: it moves to the left only)
        for (int d = -3; d <= 3; ++d) {
            const uint32_t l0 = b.at();
            std::string line = b.letters(3 * P + 1, 5 + (uint32_t)(d + 3));
            memcpy(&line[P - 3 + d], e1, 7);
            memcpy(&line[2 * P - 3 + d], e2, 7);
            memcpy(&line[3 * P - 3 + (d < 0 ? d : 0)], e3, 4);
            b.raw(line + "\n");
            b.pattern(l0 + 20, 12, 3, always);                              // a short hit of the long line
            if (d == 0) b.pattern(l0 + P - 100, P + 150, 2, always);        // a hit of two pieces that spans two edges
            else b.pattern(l0 + 2 * P - 8 + d, 16, 1, always);              // a short hit across an edge: its text has the pattern too
        }
        const uint32_t behind = b.line_with("192.168.0.1", 2, 2);
        b.ip(4, 8, 24);   // the token of the first line
        b.ip(behind, 11, 16);
        out.push_back(b.c);
    }
    {   // 300 ids, every third without data
        Builder b("many_ids");
        b.pattern(b.line_with("many.example", 4, 4), 12, 300, [](uint32_t k) { return k % 3 != 2; });
        b.pattern(b.line_with("few.example", 4, 4), 11, 3, [](uint32_t k) { return k != 0; });
        out.push_back(b.c);
    }
    {   // no id has data: no "data" key, in either tier
        Builder b("all_negative");
        b.pattern(b.line_with("none.example", 4, 4), 12, 4, never);
        b.pattern(b.line_with("none12.example", 4, 4), 14, 12, never);
        b.pattern(b.line_with("zero.example", 4, 4), 12, 0, never);
        out.push_back(b.c);
    }
    {   // compact IPv4 records behind full ones
        Builder b("compact_ipv4");
        b.ip(b.line_with("2001:db8::192.0.2.128", 3, 3), 21, 48);
        b.pattern(b.line_with("mixed.example", 3, 3), 13, 2, always);
        b.ip(b.line_with("::ffff:1.2.3.4", 3, 3), 14, 104);
        b.next_value = 0x40;   // compact records carry 22 bits of data offset
        for (const char* t : {"1.2.3.4", "10.20.30.40", "255.255.255.255", "100.64.0.1"}) b.ip(b.line_with(t, 7, 2), (uint32_t)strlen(t), (uint8_t)(8 + strlen(t)), true);
        out.push_back(b.c);
    }
    {   // per-segment sources that need escaping, line bases above 2^32, an empty segment
        Builder b("segments");
        b.c.seg_starts.push_back(0);
        b.pattern(b.line_with("seg0.example", 3, 3), 12, 1, always);
        b.ip(b.line_with("10.0.0.1", 3, 3), 8, 8);
        b.c.seg_starts.push_back(b.at());
        b.c.seg_starts.push_back(b.at());   // the one in front is empty
        b.raw("no hit here\n");
        b.ip(b.line_with("10.0.0.2", 3, 3), 8, 32);
        b.c.seg_starts.push_back(b.at());
        b.raw("\n");
        b.pattern(b.line_with("seg3.example", 3, 3), 12, 2, always);
        b.c.sources = {"dir/a \"quoted\".log", "empty", "back\\slash\ttab", std::string("ctl\x01\x7f") + "\xc3\xa9"};
        b.c.line_bases = {(1ull << 32) + 7, 0, (1ull << 40), 18446744073709551000ull};
        out.push_back(b.c);
    }
    {   // IPv6 results whose text does not parse: the fallback "cidr"
        Builder b("ipv6_fallback");
        b.ip(b.line_with("1::2::3", 3, 3), 7, 64);
        b.ip(b.line_with("fe80::1%e\"0", 3, 3), 11, 10);
        b.ip(b.line_with("fe80::1", 3, 3), 7, 10);
        out.push_back(b.c);
    }
    {   // an empty line and an unterminated last line, whose last byte is the last byte of the allocation
        Builder b("short_lines");
        b.raw("first\n");
        b.pattern(b.at(), 0, 1, always);   // a hit of no bytes on the empty line
        b.raw("\n");
        b.raw("tail\r\n");
        b.pattern(b.line_with("last.example", 2, 0, false) , 12, 1, always);
        b.c.batch.pop_back();   // line_with put a blank behind the token
        out.push_back(b.c);
    }
    {   // few source bytes, but a payload beyond RENDER_SHORT_TEXT: the record leaves the lane tier; its neighbours stay
        Builder b("big_payload");
        b.ip(b.line_with("10.0.0.1", 3, 3), 8, 8);
        const uint32_t at = b.line_with("big.example", 3, 3);
        b.pattern(at, 11, 2, always);
        b.c.payloads[(uint32_t)b.c.data_offsets.back()] = "{\"big\":\"" + b.letters(RENDER_SHORT_TEXT + 100, 1) + "\"}";
        b.ip(b.line_with("10.0.0.2", 3, 3), 8, 8);
        const uint32_t edge = b.line_with("edge.example", 3, 3);   // exactly RENDER_SHORT_TEXT bytes of text: still a lane's
        b.pattern(edge, 12, 1, always);
        b.c.payloads[(uint32_t)b.c.data_offsets.back()] = "";
        const std::string bare = model_of(b.c).text;   // the last record with an empty payload: what is missing to the bound is the payload
        const size_t last = bare.size() - (bare.rfind('\n', bare.size() - 2) + 1);
        b.c.payloads[(uint32_t)b.c.data_offsets.back()] = "\"" + b.letters(RENDER_SHORT_TEXT - (uint32_t)last - 2, 4) + "\"";
        out.push_back(b.c);
    }
    {   // no records at all
        Builder b("zero_records");
        b.raw("nothing matched\n");
        out.push_back(b.c);
    }
    for (uint32_t flags : {0u, R::FLAG_LINE_NUMBERS}) {   // without "input_line" the line's length does not count: a hit in a long line is short
        Builder b(flags ? "line_numbers" : "no_line_keys");
        b.c.flags = flags;
        b.c.line_bases = {41};
        b.c.sources = {"plain.log"};
        b.raw(b.letters(2000, 3) + " ");
        b.ip(b.at(), 7, 24); b.raw("9.8.7.6 \n");
        b.pattern(b.line_with(b.letters(RENDER_SHORT_MAX + 1, 9), 2, 2), RENDER_SHORT_MAX + 1, 1, always);   // long by its hit alone
        b.pattern(b.line_with("x.example", 2, 2), 9, 9, always);
        out.push_back(b.c);
    }
    {   // more records than one workgroup of the prefix sum covers, long ones among them
        Builder b("many_records");
        for (uint32_t k = 0; k < 2 * RENDER_SCAN_CHUNK + 77; ++k) {
            if (k % 1000 == 500) b.pattern(b.line_with("long" + std::to_string(k) + ".example", 300, 300), 12 + (uint32_t)std::to_string(k).size(), 1, always);
            else if (k % 3 == 0) { const std::string t = "10.0." + std::to_string(k / 250) + "." + std::to_string(k % 250); b.ip(b.line_with(t, k % 17, k % 5), (uint32_t)t.size(), 24); }
            else b.pattern(b.line_with("h" + std::to_string(k) + ".example", k % 13, k % 7), 9 + (uint32_t)std::to_string(k).size(), 1 + k % 3, [k](uint32_t j) { return (j + k) % 4 != 0; });
        }
        // the payloads of this case repeat: few distinct offsets under many records
        std::map<uint32_t, uint32_t> fold;
        std::map<uint32_t, std::string> kept;
        for (auto& kv : b.c.payloads) { const uint32_t to = 0x100 + 24 * (kv.first % 97); fold[kv.first] = to; kept[to] = "{\"p\":" + std::to_string(kv.first % 97) + "}"; }
        for (int64_t& d : b.c.data_offsets) if (d >= 0) d = fold[(uint32_t)d];
        for (HostRec& h : b.c.fin) if (h.kind == 2) h.value = fold[h.value];
        b.c.payloads = kept;
        out.push_back(b.c);
    }
    return out;
}

// ------------------------------------------------------------------------------------------------ one case on the device
struct Table {
    std::vector<PayloadSlot> slots;
    std::vector<uint8_t> pool;
    explicit Table(const std::map<uint32_t, std::string>& payloads) {
        uint32_t n = 8;
        while (n < 2 * payloads.size()) n *= 2;
        slots.assign(n, PayloadSlot{RENDER_KEY_EMPTY, 0, 0, 0});
        for (const auto& kv : payloads) {
            uint32_t s = payload_slot(kv.first, n);
            while (slots[s].key != RENDER_KEY_EMPTY) s = (s + 1) & (n - 1);
            slots[s] = PayloadSlot{kv.first, (uint32_t)pool.size(), (uint32_t)kv.second.size(), 0};
            pool.insert(pool.end(), kv.second.begin(), kv.second.end());
        }
    }
};

static int failed = 0, n_cases = 0;
static void verdict(const char* kind, const Case& c, const std::string& fields, const std::string& err) {
    ++n_cases;
    if (!err.empty()) ++failed;
    printf("%s %s %s %s\n", kind, c.name.c_str(), fields.c_str(), err.empty() ? "OK" : ("FAIL: " + err).c_str());
    fflush(stdout);
}

static void run_case(const Case& c) {
    const Model m = model_of(c);
    const uint32_t n_fin = (uint32_t)c.fin.size(), n_c4 = (uint32_t)c.c4.size(), n = n_fin + n_c4;
    // device images
    std::vector<uint8_t> batch(c.batch.begin(), c.batch.end());
    Dev<uint8_t> d_batch(batch);   // exactly the batch
    std::vector<uint4> fin;
    for (const HostRec& h : c.fin) fin.push_back(make_uint4(h.start, h.len | (3u << 24), h.value, (uint32_t)h.kind | ((uint32_t)h.prefix << 8) | ((uint32_t)h.n_ids << 16)));
    std::vector<uint2> c4;
    for (const HostRec& h : c.c4) c4.push_back(make_uint2(h.start, h.value | ((h.len - 7u) << 22) | ((uint32_t)h.prefix << 26)));
    Dev<uint4> d_fin(fin);
    Dev<uint2> d_c4(c4);
    Dev<int64_t> d_offs(c.data_offsets);
    Dev<LineRec> d_fin_lines(m.fin_lines), d_c4_lines(m.c4_lines);
    Dev<uint32_t> d_seg_fin(m.seg_of_fin), d_seg_c4(m.seg_of_c4), d_seg_base(m.seg_line_base);
    Dev<RenderSource> d_sources(m.sources);
    Dev<uint8_t> d_source_text(std::vector<uint8_t>(m.source_text.begin(), m.source_text.end()));
    Dev<uint64_t> d_bases(c.line_bases);
    const Table table(c.payloads);
    Dev<PayloadSlot> d_slots(table.slots);
    Dev<uint8_t> d_pool(table.pool);

    RenderInput in;
    in.b = HitBatch{d_batch.p, (uint32_t)batch.size(), d_fin.p, n_fin, d_c4.p, n_c4};
    in.data_offsets = d_offs.p; in.n_data_offsets = (uint32_t)c.data_offsets.size();
    in.flags = c.flags;
    if (c.flags) { in.fin_lines = d_fin_lines.p; in.c4_lines = d_c4_lines.p; }
    in.n_segments = (uint32_t)c.seg_starts.size();
    if (in.n_segments) { in.seg_of_fin = d_seg_fin.p; in.seg_of_c4 = d_seg_c4.p; in.seg_line_base = d_seg_base.p; }
    in.sources = d_sources.p; in.source_text = d_source_text.p; in.line_bases = d_bases.p;

    uint32_t set_slots = 64;
    while (set_slots < 4 * (c.data_offsets.size() + n)) set_slots *= 2;
    Dev<uint64_t> d_len(n), d_off((size_t)n + 1), d_chunks(render_chunks(n));
    Dev<RenderLong> d_long(n);
    Dev<uint32_t> d_set(set_slots);
    Dev<RenderCounters> d_ctr(1);
    Dev<RenderMissCounter> d_miss(1);

    auto work = [&](Dev<uint32_t>& piece_len, Dev<uint64_t>& piece_off, uint32_t piece_cap, Dev<uint32_t>& list, uint32_t miss_cap, uint32_t long_hint, uint32_t slots = 0) {
        RenderWork w{};
        w.long_hint = long_hint;
        w.rec_len = d_len.p; w.rec_off = d_off.p; w.chunk_sums = d_chunks.p; w.long_list = d_long.p;
        w.piece_len = piece_len.p; w.piece_off = piece_off.p; w.piece_cap = piece_cap;
        w.miss_set = d_set.p; w.miss_set_slots = slots ? slots : set_slots; w.miss_list = list.p; w.miss_cap = miss_cap;
        w.ctr = d_ctr.p; w.miss = d_miss.p;
        d_ctr.fill(0); d_miss.fill(0); d_set.fill(0xFF);
        return w;
    };
    Dev<uint32_t> d_piece_len(m.n_pieces + 8);
    Dev<uint64_t> d_piece_off(m.n_pieces + 8);
    char fields[256];

    // MISS: the table empty
    const uint32_t want_misses = (uint32_t)m.offsets.size();
    std::vector<uint32_t> miss_caps{0};
    if (want_misses) { if (want_misses > 1) miss_caps.push_back(want_misses - 1); miss_caps.push_back(want_misses); }
    for (uint32_t cap : miss_caps) {
        Dev<uint32_t> d_list(cap + LIST_GUARD);
        d_list.fill(POISON);
        const RenderWork w = work(d_piece_len, d_piece_off, m.n_pieces + 8, d_list, cap, 0);   // no hint: one workgroup serves the long list
        HIP_OK(render_measure(in, PayloadTable{nullptr, 0, nullptr}, w, ~0ull, N_CU, nullptr));
        HIP_OK(hipDeviceSynchronize());
        const uint32_t misses = d_miss.host()[0].misses;
        const std::vector<uint32_t> list = d_list.host();
        std::string err;
        if (misses != want_misses) err = "misses " + std::to_string(misses) + ", model " + std::to_string(want_misses);
        std::set<uint32_t> seen;
        for (uint32_t k = 0; k < std::min(cap, misses) && err.empty(); ++k)
            if (!m.offsets.count(list[k]) || !seen.insert(list[k]).second) err = "entry " + std::to_string(k) + " of the list is foreign or repeated";
        for (uint32_t k = cap; k < cap + LIST_GUARD && err.empty(); ++k) if (list[k] != 0xA5A5A5A5u) err = "store behind the capacity of the miss list";
        snprintf(fields, sizeof(fields), "cap=%u misses=%u", cap, misses);
        verdict("MISS", c, fields, err);
    }

    // a set of two slots: lanes that find no slot append without a claim. The list then repeats offsets, and still holds nothing else
    if (want_misses) {
        const uint32_t cap = (uint32_t)(c.data_offsets.size() + n);   // every lookup could append
        Dev<uint32_t> d_list(cap + LIST_GUARD);
        d_list.fill(POISON);
        const RenderWork w = work(d_piece_len, d_piece_off, m.n_pieces + 8, d_list, cap, m.n_long, 2);
        HIP_OK(render_measure(in, PayloadTable{nullptr, 0, nullptr}, w, ~0ull, N_CU, nullptr));
        HIP_OK(hipDeviceSynchronize());
        const uint32_t misses = d_miss.host()[0].misses;
        const std::vector<uint32_t> list = d_list.host();
        std::string err;
        std::set<uint32_t> seen;
        if (misses < want_misses || misses > cap) err = "misses " + std::to_string(misses) + ", model " + std::to_string(want_misses) + " .. " + std::to_string(cap);
        for (uint32_t k = 0; k < misses && err.empty(); ++k) { if (!m.offsets.count(list[k])) err = "a foreign entry"; seen.insert(list[k]); }
        if (err.empty() && seen != m.offsets) err = "the list does not hold every offset";
        for (uint32_t k = cap; k < cap + LIST_GUARD && err.empty(); ++k) if (list[k] != 0xA5A5A5A5u) err = "store behind the capacity of the miss list";
        snprintf(fields, sizeof(fields), "slots=2 misses=%u", misses);
        verdict("CROWDED", c, fields, err);
    }

    // CASE: the table filled
    const PayloadTable pt{d_slots.p, (uint32_t)table.slots.size(), d_pool.p};
    const uint64_t demand = m.text.size();
    std::vector<uint64_t> caps{0, demand ? demand - 1 : 1};
    if (demand) { caps.push_back(demand); caps.push_back(demand + 1); caps.push_back(2 * demand); }
    for (uint64_t cap : caps) {
        Dev<uint32_t> d_list(LIST_GUARD);
        const RenderWork w = work(d_piece_len, d_piece_off, m.n_pieces + 8, d_list, 0, cap == demand ? 0 : m.n_long);   // with and without the hint
        const uint64_t room = std::max(cap, demand);
        Dev<uint8_t> d_text(GUARD + room + GUARD);
        d_text.fill(POISON);
        HIP_OK(render_measure(in, pt, w, ~0ull, N_CU, nullptr));
        HIP_OK(render_write(in, pt, w, d_text.p + GUARD, cap, N_CU, nullptr));
        HIP_OK(hipDeviceSynchronize());
        const RenderCounters ctr = d_ctr.host()[0];
        const uint32_t misses = d_miss.host()[0].misses;
        const std::vector<uint8_t> got = d_text.host();
        std::string err;
        if (ctr.demand != demand) err = "demand " + std::to_string(ctr.demand) + ", model " + std::to_string(demand);
        else if (misses) err = std::to_string(misses) + " misses with the table filled";
        else if (ctr.status != RENDER_OK || ctr.pieces_short) err = "status " + std::to_string(ctr.status) + " pieces_short " + std::to_string(ctr.pieces_short);
        else if (ctr.n_short != m.n_short || ctr.n_long != m.n_long || ctr.n_pieces != m.n_pieces)
            err = "tiers " + std::to_string(ctr.n_short) + "/" + std::to_string(ctr.n_long) + "/" + std::to_string(ctr.n_pieces) + ", model " + std::to_string(m.n_short) + "/" +
                  std::to_string(m.n_long) + "/" + std::to_string(m.n_pieces);
        const uint64_t end = std::min(cap, demand);
        for (uint64_t k = 0; k < GUARD && err.empty(); ++k) if (got[k] != POISON) err = "store in front of the block, at -" + std::to_string(GUARD - k);
        for (uint64_t k = end; k < room + GUARD && err.empty(); ++k) if (got[GUARD + k] != POISON) err = "store at or behind min(demand, capacity), at " + std::to_string(k);
        for (uint64_t k = 0; k < end && err.empty(); ++k)
            if (got[GUARD + k] != (uint8_t)m.text[k]) err = "byte " + std::to_string(k) + " is " + std::to_string(got[GUARD + k]) + ", model " + std::to_string((uint8_t)m.text[k]);
        if (err.empty() && n) {   // the offsets of the records
            const std::vector<uint64_t> off = d_off.host();
            if (off[0] != 0 || off[n] != demand) err = "rec_off does not span the block";
            for (uint32_t i = 0; i < n && err.empty(); ++i) if (off[i] >= off[i + 1] || m.text[off[i + 1] - 1] != '\n' || m.text[off[i]] != '{') err = "rec_off[" + std::to_string(i) + "]";
        }
        snprintf(fields, sizeof(fields), "cap=%llu demand=%llu records=%u short=%u long=%u pieces=%u", (unsigned long long)cap, (unsigned long long)ctr.demand, n, ctr.n_short,
                 ctr.n_long, (uint32_t)ctr.n_pieces);
        verdict("CASE", c, fields, err);
    }

    // SWEEP: every capacity in a range around three record boundaries, most of them no multiple of 16 and most of them inside a
    // record: the write step of a block that is too small ends in the middle of a wave's records, and the records behind the end
    // begin inside the 16-byte unit the end cuts
    if (n >= 2) {
        std::vector<uint64_t> bounds;
        for (size_t k = 0; k + 1 < m.text.size(); ++k) if (m.text[k] == '\n') bounds.push_back(k + 1);   // where a record begins
        std::set<uint64_t> sweep;
        // where a wave's run of short records begins: record 64, 128, ... (a wave takes 64 records), 2048 (a workgroup boundary
        // as well), and the record behind a long one — in a case of few records simply every record
        std::vector<uint64_t> around;
        if (n <= 16) around = bounds;
        else for (size_t k : {(size_t)0, (size_t)63, (size_t)127, (size_t)2047, bounds.size() / 2, bounds.size() - 1}) if (k < bounds.size()) around.push_back(bounds[k]);
        for (uint64_t b0 : around)
            for (uint64_t cap = b0 > 40 ? b0 - 40 : 0; cap <= b0 + 40 && cap < demand; ++cap) sweep.insert(cap);
        Dev<uint32_t> d_list(LIST_GUARD);
        Dev<uint8_t> d_text(GUARD + demand + GUARD);
        std::string err;
        for (uint64_t cap : sweep) {
            const RenderWork w = work(d_piece_len, d_piece_off, m.n_pieces + 8, d_list, 0, m.n_long);
            d_text.fill(POISON);
            HIP_OK(render_measure(in, pt, w, ~0ull, N_CU, nullptr));
            HIP_OK(render_write(in, pt, w, d_text.p + GUARD, cap, N_CU, nullptr));
            HIP_OK(hipDeviceSynchronize());
            const std::vector<uint8_t> got = d_text.host();
            if (d_ctr.host()[0].demand != demand) err = "demand at capacity " + std::to_string(cap);
            for (uint64_t k = 0; k < GUARD && err.empty(); ++k) if (got[k] != POISON) err = "capacity " + std::to_string(cap) + ": store in front of the block";
            for (uint64_t k = cap; k < demand + GUARD && err.empty(); ++k) if (got[GUARD + k] != POISON) err = "capacity " + std::to_string(cap) + ": store behind it, at " + std::to_string(k);
            for (uint64_t k = 0; k < cap && err.empty(); ++k) if (got[GUARD + k] != (uint8_t)m.text[k]) err = "capacity " + std::to_string(cap) + ": byte " + std::to_string(k);
            if (!err.empty()) break;
        }
        snprintf(fields, sizeof(fields), "caps=%zu", sweep.size());
        verdict("SWEEP", c, fields, err);
    }

    // PIECES: one slot short
    if (m.n_pieces) {
        Dev<uint32_t> d_list(LIST_GUARD), short_len(m.n_pieces - 1 + LIST_GUARD);
        Dev<uint64_t> short_off(m.n_pieces - 1 + LIST_GUARD);
        short_len.fill(POISON); short_off.fill(POISON);
        const RenderWork w = work(short_len, short_off, m.n_pieces - 1, d_list, 0, m.n_long);
        Dev<uint8_t> d_text(GUARD + demand + GUARD);
        d_text.fill(POISON);
        HIP_OK(render_measure(in, pt, w, ~0ull, N_CU, nullptr));
        HIP_OK(render_write(in, pt, w, d_text.p + GUARD, demand, N_CU, nullptr));
        HIP_OK(hipDeviceSynchronize());
        const RenderCounters ctr = d_ctr.host()[0];
        std::string err;
        if (!ctr.pieces_short) err = "the pass did not notice";
        else if (ctr.n_pieces != m.n_pieces) err = "piece demand " + std::to_string(ctr.n_pieces) + ", model " + std::to_string(m.n_pieces);
        const std::vector<uint8_t> got = d_text.host();
        for (size_t k = 0; k < got.size() && err.empty(); ++k) if (got[k] != POISON) err = "a store to the block";
        const std::vector<uint32_t> pl = short_len.host();
        const std::vector<uint64_t> po = short_off.host();
        for (uint32_t k = m.n_pieces - 1; k < pl.size() && err.empty(); ++k) if (pl[k] != 0xA5A5A5A5u || po[k] != 0xA5A5A5A5A5A5A5A5ull) err = "store behind the capacity of the piece arrays";
        snprintf(fields, sizeof(fields), "cap=%u pieces=%u", m.n_pieces - 1, (uint32_t)ctr.n_pieces);
        verdict("PIECES", c, fields, err);
    }

    // a block limit below the demand: RENDER_TOO_LARGE, nothing stored
    if (demand > 64) {
        Dev<uint32_t> d_list(LIST_GUARD);
        const RenderWork w = work(d_piece_len, d_piece_off, m.n_pieces + 8, d_list, 0, m.n_long);
        Dev<uint8_t> d_text(GUARD + demand + GUARD);
        d_text.fill(POISON);
        HIP_OK(render_measure(in, pt, w, 64, N_CU, nullptr));
        HIP_OK(render_write(in, pt, w, d_text.p + GUARD, demand, N_CU, nullptr));
        HIP_OK(hipDeviceSynchronize());
        const RenderCounters ctr = d_ctr.host()[0];
        std::string err;
        if (ctr.status != RENDER_TOO_LARGE) err = "status " + std::to_string(ctr.status);
        else if (ctr.demand != demand) err = "demand " + std::to_string(ctr.demand);
        const std::vector<uint8_t> got = d_text.host();
        for (size_t k = 0; k < got.size() && err.empty(); ++k) if (got[k] != POISON) err = "a store to the block";
        snprintf(fields, sizeof(fields), "max=64 demand=%llu", (unsigned long long)ctr.demand);
        verdict("LIMIT", c, fields, err);
    }
}

int main() {
    for (const Case& c : cases()) run_case(c);
    printf("DONE cases=%d failed=%d\n", n_cases, failed);
    return failed ? 1 : 0;
}
