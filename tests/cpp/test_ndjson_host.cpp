// csrc/ndjson_host.cpp driven without a GPU, against an assembly of the records written out here from the host code that exists:
// json_escape, utf8_lossy_append, format_cidr(parse_ip()) and snprintf — never render::record_emit. Payloads come from a map in this
// file. Built with -fsanitize=address,undefined (tests/test_ndjson_host.py): every input array and the batch text lie in heap blocks of
// exactly their length, so a load outside one stops the program.
//   test_ndjson_host cases | big
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "data_codec.h"
#include "ndjson_host.h"
#include "netaddr.h"
#include "utf8_lossy.h"

using namespace mxy;
namespace N = mxy::ndjson;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                     \
    } while (0)

// ------------------------------------------------------------------------------------------------ payloads
static const std::map<uint32_t, std::string> PAYLOADS = {{8, "{\"a\":\"x\\\"y\"}"}, {40, "[1,2.5,{\"k\":{}}]"}, {99, "\"s\""}, {555, "{\"late\":true}"}};
constexpr uint32_t UNDECODABLE = 77;   // not in the map: the decode fails
static std::atomic<int> calls_555{0};
static void payload(const void* ctx, uint32_t off, std::string& json) {
    if (off == 555) calls_555.fetch_add(1);
    const auto& m = *static_cast<const std::map<uint32_t, std::string>*>(ctx);
    const auto it = m.find(off);
    json = it == m.end() ? "null" : it->second;
}
static const N::Payloads PAY{&payload, &PAYLOADS};

// ------------------------------------------------------------------------------------------------ a result in exact heap blocks
template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {   // a block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

struct Rec { uint8_t kind; uint32_t start, len; uint8_t prefix; uint32_t value; uint16_t n_ids; };
constexpr uint32_t LINE0 = 5;   // the batch stands for a cut out of a longer one: its first line has this index

struct Result {
    std::string text;
    std::vector<Rec> hits, ip4;
    std::vector<int64_t> offs;
    std::vector<uint32_t> seg_starts;
    // exact blocks
    std::unique_ptr<uint8_t[]> b_text, b_block;
    std::unique_ptr<matchy_scan_hit_t[]> b_hits;
    std::unique_ptr<matchy_scan_ip4_hit_t[]> b_ip4;
    std::unique_ptr<int64_t[]> b_offs;
    std::unique_ptr<matchy_scan_line_t[]> b_lines, b_ip4_lines;
    std::unique_ptr<uint32_t[]> b_seg_of, b_seg_of_ip4, b_line_off, b_line_no, b_line_of, b_line_of_ip4;
    std::unique_ptr<matchy_scan_segment_t[]> b_segs;
    matchy_scan_hit_lines_t block{};
    std::vector<matchy_scan_segment_t> segs;

    matchy_scan_line_t line_of(uint32_t start) const {
        uint32_t line = 0, ls = 0;
        for (uint32_t i = 0; i < start; ++i) if (text[i] == '\n') { ++line; ls = i + 1; }
        uint32_t le = ls;
        while (le < text.size() && text[le] != '\n') ++le;
        return matchy_scan_line_t{LINE0 + line, ls, le, 0};
    }
    uint32_t seg_of(uint32_t start) const {
        uint32_t s = 0;
        while (s + 1 < seg_starts.size() && seg_starts[s + 1] <= start) ++s;
        return s;
    }
    void freeze() {
        b_text.reset(new uint8_t[text.size()]);
        memcpy(b_text.get(), text.data(), text.size());
        std::vector<matchy_scan_hit_t> h;
        std::vector<matchy_scan_ip4_hit_t> c;
        std::vector<matchy_scan_line_t> hl, cl;
        std::vector<uint32_t> hs, cs;
        for (const Rec& r : hits) { h.push_back(matchy_scan_hit_t{r.start, r.len | (1u << 24), r.value, r.kind, r.prefix, r.n_ids}); hl.push_back(line_of(r.start)); hs.push_back(seg_of(r.start)); }
        for (const Rec& r : ip4) {
            CHECK(r.len >= 7 && r.len <= 15 && r.value < (1u << 22) && r.prefix <= 32, "compact record out of range");
            c.push_back(matchy_scan_ip4_hit_t{r.start, r.value | ((r.len - 7u) << 22) | ((uint32_t)r.prefix << 26)});
            cl.push_back(line_of(r.start)); cs.push_back(seg_of(r.start));
        }
        for (size_t s = 0; s < seg_starts.size(); ++s) {
            matchy_scan_segment_t g{};
            g.start = seg_starts[s]; g.len = (s + 1 < seg_starts.size() ? seg_starts[s + 1] : (uint32_t)text.size()) - g.start;
            g.line_base = LINE0;
            for (uint32_t i = 0; i < g.start; ++i) g.line_base += text[i] == '\n';
            for (uint32_t x : hs) g.hits += x == s;
            for (uint32_t x : cs) g.hits += x == s;
            segs.push_back(g);
        }
        // the block of hit lines: the distinct lines with a record, ascending, each ended by one '\n'
        std::map<uint32_t, matchy_scan_line_t> with;
        for (const auto& l : hl) with[l.line] = l;
        for (const auto& l : cl) with[l.line] = l;
        std::string bt;
        std::vector<uint32_t> off{0}, no, of, of4;
        std::map<uint32_t, uint32_t> k_of;
        for (const auto& kv : with) {
            k_of[kv.first] = (uint32_t)no.size();
            no.push_back(kv.first - LINE0);
            bt += text.substr(kv.second.line_start, kv.second.line_end - kv.second.line_start) + "\n";
            off.push_back((uint32_t)bt.size());
        }
        for (const auto& l : hl) of.push_back(k_of[l.line]);
        for (const auto& l : cl) of4.push_back(k_of[l.line]);
        b_block.reset(new uint8_t[bt.size()]);
        memcpy(b_block.get(), bt.data(), bt.size());
        b_hits = exact(h); b_ip4 = exact(c); b_offs = exact(offs); b_lines = exact(hl); b_ip4_lines = exact(cl);
        b_seg_of = exact(hs); b_seg_of_ip4 = exact(cs); b_segs = exact(segs);
        b_line_off = exact(off); b_line_no = exact(no); b_line_of = exact(of); b_line_of_ip4 = exact(of4);
        block = matchy_scan_hit_lines_t{b_block.get(), bt.size(), (uint32_t)no.size(), b_line_off.get(), b_line_no.get(), b_line_of.get(), b_line_of_ip4.get()};
    }
    // from_block: the text comes from the block of hit lines and the batch is NULL
    N::ResultView view(bool with_lines, bool with_segments, bool from_block) const {
        N::ResultView v;
        v.hits = b_hits.get(); v.n_hits = hits.size(); v.ip4_hits = b_ip4.get(); v.n_ip4_hits = ip4.size(); v.data_offsets = b_offs.get();
        if (with_lines || from_block) { v.lines = b_lines.get(); v.ip4_lines = b_ip4_lines.get(); }
        if (with_segments) { v.segment_of_hit = b_seg_of.get(); v.segment_of_ip4_hit = b_seg_of_ip4.get(); v.segments = b_segs.get(); v.n_segments = segs.size(); }
        if (from_block) v.block = &block; else v.text = b_text.get();
        return v;
    }
};

// ------------------------------------------------------------------------------------------------ the expectation
static std::string quoted(const std::string& s) { std::string o; json_escape(s, o); return o; }

// one record without its '\n'; line_keys: "" or the text of "input_line" / "line_number" with their commas
static std::string want_record(const Result& R, const Rec& r, const std::string& line_keys, const std::string& source) {
    const std::string hit = R.text.substr(r.start, r.len);
    std::string o = "{";
    if (r.kind == 2) {
        IpAddr ip;
        const std::string cidr = parse_ip(hit.data(), hit.size(), ip) ? format_cidr(ip, r.prefix) : hit + "/" + std::to_string((unsigned)r.prefix);
        const auto p = PAYLOADS.find(r.value);
        o += "\"cidr\":" + quoted(cidr) + ",\"data\":" + (p == PAYLOADS.end() ? std::string("null") : p->second) + "," + line_keys + "\"match_type\":\"ip\",\"matched_text\":" + quoted(hit);
        o += ",\"prefix_len\":" + std::to_string((unsigned)r.prefix);
    } else {
        std::string arr;
        for (uint32_t k = 0; k < r.n_ids; ++k) {
            const int64_t off = R.offs[r.value + k];
            if (off < 0) continue;
            const auto p = PAYLOADS.find((uint32_t)off);
            arr += (arr.empty() ? "" : ",") + (p == PAYLOADS.end() ? std::string("null") : p->second);
        }
        if (!arr.empty()) o += "\"data\":[" + arr + "],";
        o += line_keys + "\"match_type\":\"pattern\",\"matched_text\":" + quoted(hit) + ",\"pattern_count\":" + std::to_string((unsigned)r.n_ids);
    }
    return o + ",\"source\":" + quoted(source) + ",\"timestamp\":\"0.000\"}";
}
static std::string want_line_keys(const Result& R, const Rec& r, bool input_line, uint64_t base) {
    const matchy_scan_line_t l = R.line_of(r.start);
    std::string o;
    if (input_line) {
        std::string lossy;
        utf8_lossy_append(reinterpret_cast<const uint8_t*>(R.text.data()) + l.line_start, l.line_end - l.line_start, lossy);
        o += "\"input_line\":" + quoted(lossy) + ",";
    }
    char num[32];
    snprintf(num, sizeof(num), "%llu", (unsigned long long)(base + l.line + 1));
    return o + "\"line_number\":" + num + ",";
}
// the whole text of a result. sources: per segment, with line_bases when lines are asked for
static std::string want_text(const Result& R, bool lines, bool input_line, uint64_t line_base, const char* source, const std::vector<const char*>* sources,
                             const std::vector<uint64_t>* line_bases) {
    std::string o;
    for (int pass = 0; pass < 2; ++pass)
        for (const Rec& r : pass ? R.ip4 : R.hits) {
            const uint32_t s = R.seg_of(r.start);
            const uint64_t base = sources ? (*line_bases)[s] - R.segs[s].line_base : line_base;
            const char* src = sources ? (*sources)[s] : source;
            o += want_record(R, r, lines ? want_line_keys(R, r, input_line, base) : "", src ? src : "-") + "\n";
        }
    return o;
}

static std::string rendered(N::Renderer& rn, const N::ResultView& v, const N::Keys& k, int32_t want_rc = MATCHY_SUCCESS, std::string* error = nullptr) {
    char* out = nullptr;
    size_t n = 0;
    std::string err;
    const int32_t rc = rn.render(v, k, PAY, &out, &n, err);
    CHECK(rc == want_rc, "render returned %d (%s), expected %d", rc, err.c_str(), want_rc);
    if (error) *error = err;
    if (rc != MATCHY_SUCCESS) return "";
    CHECK(out && out[n] == 0, "no NUL behind the text");
    std::string s(out, n);
    free(out);
    return s;
}
static void same(const std::string& got, const std::string& want, const char* what) {
    size_t d = 0;
    while (d < got.size() && d < want.size() && got[d] == want[d]) ++d;
    CHECK(got == want, "%s: differs at byte %zu of %zu / %zu:\n got  %s\n want %s", what, d, got.size(), want.size(), got.substr(d > 40 ? d - 40 : 0, 160).c_str(),
          want.substr(d > 40 ? d - 40 : 0, 160).c_str());
}

// ------------------------------------------------------------------------------------------------ the small cases
static Result small_result() {
    Result R;
    auto at = [&](const char* needle) { const size_t p = R.text.find(needle); if (p == std::string::npos) { printf("no %s\n", needle); exit(2); } return (uint32_t)p; };
    R.text = std::string("from 10.1.2.3 \"q\" 192.168.100.200\r\n"        // segment 0: IPv4 in hits and a compact one, '"' and '\r' in the line
                         "x 2001:db8::1 \xff\xe0\xa0\n"                    // IPv6; ill-formed UTF-8 in the line
                         "bad 1::2::3 here\n"                              // a kind-2 record whose text does not parse; its payload does not decode
                         "nothing on this line\n"                          // segment 1 owns no record
                         "\tGET evil\"\\.ex\x01\x7f\x80\xc3\xa9 end\n"     // segment 2: '"', '\\', a control byte, 0x7F, bytes >= 0x80 in the matched text
                         "none.example uno.example zero\n"
                         "all.three\n"
                         "tail 10.9.8.7 \xf0\x90");                       // the last line has no terminator and ends inside a sequence
    R.seg_starts = {0, at("nothing"), at("\tGET")};
    R.offs = {8, -1, 99, -1, -1, 40, 8, 40, 99, UNDECODABLE};
    R.hits = {
        {2, at("10.1.2.3"), 8, 24, 8, 0},
        {2, at("2001:db8::1"), 11, 33, 40, 0},
        {2, at("1::2::3"), 7, 128, UNDECODABLE, 0},
        {3, at("evil"), (uint32_t)strlen("evil\"\\.ex\x01\x7f\x80\xc3\xa9"), 0, 0, 3},   // some of the offsets are -1
        {3, at("none.example"), 12, 0, 3, 2},                                          // all are -1: no "data" key
        {3, at("uno.example"), 11, 0, 5, 1},
        {3, at("zero"), 4, 0, 0, 0},
        {3, at("all.three"), 9, 0, 6, 4},                                              // none is -1; the last one does not decode
    };
    R.ip4 = {{2, at("192.168.100.200"), 15, 16, 40, 0}, {2, at("10.9.8.7"), 8, 32, 8, 0}};
    R.freeze();
    return R;
}

static void test_cases() {
    const Result R = small_result();
    const std::vector<const char*> sources = {"a \"b\".log", "unused\\", nullptr};
    const std::vector<uint64_t> bases = {100, 7, 4000000000ull};
    size_t n = 0;
    for (int from_block = 0; from_block < 2; ++from_block) {
        N::Renderer rn;
        const char* what = from_block ? "from the block" : "from the batch";
        // no line keys, twice: the second time the payloads and the source come from the cache
        for (int again = 0; again < 2; ++again) same(rendered(rn, R.view(false, false, from_block), N::Keys{"p\\q", nullptr, false, false, 0, nullptr}), want_text(R, false, false, 0, "p\\q", nullptr, nullptr), what);
        CHECK(rn.cached(8) && rn.cached(40) && rn.cached(99) && rn.cached(UNDECODABLE), "payloads are not in the cache");
        same(rendered(rn, R.view(false, false, from_block), N::Keys{}), want_text(R, false, false, 0, nullptr, nullptr, nullptr), what);
        // line numbers with a base; then with input lines
        same(rendered(rn, R.view(true, false, from_block), N::Keys{"s", nullptr, true, false, 1000, nullptr}), want_text(R, true, false, 1000, "s", nullptr, nullptr), what);
        same(rendered(rn, R.view(true, false, from_block), N::Keys{"s", nullptr, true, true, (1ull << 40), nullptr}), want_text(R, true, true, 1ull << 40, "s", nullptr, nullptr), what);
        // with_input_line without lines: no line keys
        same(rendered(rn, R.view(true, false, from_block), N::Keys{"s", nullptr, false, true, 9, nullptr}), want_text(R, false, false, 0, "s", nullptr, nullptr), what);
        // segments: sources alone, then with per-segment bases
        same(rendered(rn, R.view(false, true, from_block), N::Keys{nullptr, sources.data(), false, false, 0, nullptr}), want_text(R, false, false, 0, nullptr, &sources, &bases), what);
        same(rendered(rn, R.view(true, true, from_block), N::Keys{nullptr, sources.data(), true, true, 0, bases.data()}), want_text(R, true, true, 0, nullptr, &sources, &bases), what);
        n += 8;
        // the single-record call: the bulk line without its '\n' and line keys
        for (int pass = 0; pass < 2; ++pass) {
            const std::vector<Rec>& recs = pass ? R.ip4 : R.hits;
            for (size_t i = 0; i < recs.size(); ++i) {
                std::string one;
                CHECK(N::Renderer::record(R.view(false, false, from_block), !pass, i, "one \"src\"", PAY, one), "record %zu has no text", i);
                same(one, want_record(R, recs[i], "", "one \"src\""), "single record");
                ++n;
            }
        }
    }
    // neither the block nor the batch: the single-record call has nothing to read
    N::ResultView bare = R.view(false, false, false);
    bare.text = nullptr;
    std::string one;
    CHECK(!N::Renderer::record(bare, true, 0, nullptr, PAY, one), "a record without text was rendered");
    // hits == NULL with a count (a counts-only fetch): empty text
    N::Renderer rn;
    N::ResultView counts;
    counts.n_hits = 3;
    same(rendered(rn, counts, N::Keys{}), "", "counts only");
    // refusals
    std::string err;
    rendered(rn, R.view(false, false, false), N::Keys{"s", nullptr, true, false, 0, nullptr}, MATCHY_ERROR_INVALID_PARAM, &err);
    CHECK(err == "matchy_scan_result_to_ndjson_lines: the result has no line records", "refusal: %s", err.c_str());
    N::ResultView short_table = R.view(false, true, false);
    short_table.n_segments = 2;   // records of segment 2 now point outside the table
    rendered(rn, short_table, N::Keys{nullptr, sources.data(), false, false, 0, nullptr}, MATCHY_ERROR_OUT_OF_MEMORY, &err);
    CHECK(err == "matchy_scan_result_to_ndjson_segments: a segment index lies outside the table", "refusal: %s", err.c_str());
    N::ResultView no_indices = R.view(false, false, false);
    rendered(rn, no_indices, N::Keys{nullptr, sources.data(), false, false, 0, nullptr}, MATCHY_ERROR_INVALID_PARAM, &err);
    CHECK(err == "matchy_scan_result_to_ndjson_segments: the result has no segment indices", "refusal: %s", err.c_str());
    printf("cases=%zu\n", n);
}

// 2 * 16384 + 1 records: two pieces where MATCHY_AMD_JSON_THREADS allows them. Payload 555 belongs to one record of each half and is
// in no cache before, so with two pieces both render it themselves.
static void test_big() {
    Result R;
    R.text = "a 10.1.2.3 b\nc 2001:db8::1 d \xe2\x82\n";
    const uint32_t v4 = (uint32_t)R.text.find("10.1"), v6 = (uint32_t)R.text.find("2001");
    const size_t n = 2 * 16384 + 1;
    for (size_t i = 0; i < n; ++i) {
        const bool late = i == 5 || i == n - 5;
        if (i % 3) R.hits.push_back({2, v4, 8, (uint8_t)(i % 33), late ? 555u : 8u, 0});
        else R.hits.push_back({2, v6, 11, (uint8_t)(i % 129), late ? 555u : 40u, 0});
    }
    R.seg_starts = {0};
    R.freeze();
    N::Renderer rn;
    CHECK(!rn.cached(555), "the cache is not empty");
    const std::string got = rendered(rn, R.view(true, false, false), N::Keys{"big", nullptr, true, true, 0, nullptr});
    same(got, want_text(R, true, true, 0, "big", nullptr, nullptr), "big");
    CHECK(rn.cached(555) && rn.cached(8) && rn.cached(40), "fresh payloads did not join the cache");
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : got) h = (h ^ c) * 1099511628211ull;
    printf("big records=%zu bytes=%zu fnv=%016llx payload_555_calls=%d\n", n, got.size(), (unsigned long long)h, calls_555.load());
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    if (what == "all" || what == "cases") test_cases();
    if (what == "all" || what == "big") test_big();
    if (failures) { printf("ndjson_host FAILED: %d\n", failures); return 1; }
    printf("ndjson_host ok\n");
    return 0;
}
