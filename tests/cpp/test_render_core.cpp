// csrc/render_core.h driven sequentially, against the host code that exists: utf8_lossy_append + json_escape for the two escaped
// fields, format_cidr(parse_ip()) and an snprintf formatter written out here for the addresses, snprintf for the numbers, and a
// std::string assembly of whole records. Built with -fsanitize=address,undefined (tests/test_render_core_host.py): every field lies
// in a heap block of exactly its length and every output in a block of exactly the measured length, so a load outside a field or a
// store behind the measured length stops the program.
//   test_render_core escape | window | random | ip | decimal | records
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "data_codec.h"
#include "render_core.h"
#include "utf8_lossy.h"

using namespace mxy;
namespace R = mxy::render;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                     \
    } while (0)

static std::string hex(const std::string& s) {
    std::string o;
    char b[4];
    for (unsigned char c : s) { snprintf(b, sizeof(b), "%02x", c); o += b; }
    return o;
}

// a heap block of exactly s.size() bytes (size 0: a block of one byte that is never handed out as readable)
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    uint32_t n;
    explicit Exact(const std::string& s) : p(new uint8_t[s.size()]), n((uint32_t)s.size()) { memcpy(p.get(), s.data(), s.size()); }
};

static std::string host_text(const std::string& s) {   // json_escape without its quotes
    std::string o;
    json_escape(s, o);
    return o.substr(1, o.size() - 2);
}
static std::string host_line(const std::string& s) {
    std::string lossy;
    utf8_lossy_append(reinterpret_cast<const uint8_t*>(s.data()), s.size(), lossy);
    return host_text(lossy);
}

// bytes [a, b) of the field through the per-byte rules, into a block of exactly the measured length
static std::string piece(const Exact& f, bool as_line, uint32_t a, uint32_t b) {
    const uint64_t len = as_line ? R::line_piece_len(f.p.get(), f.n, a, b) : R::text_piece_len(f.p.get(), a, b);
    std::unique_ptr<uint8_t[]> out(new uint8_t[len]);
    uint8_t t[R::BYTE_TEXT_MAX];
    uint64_t at = 0;
    for (uint32_t i = a; i < b; ++i) {
        const uint32_t k = as_line ? R::line_byte_put(f.p.get(), f.n, i, t) : R::esc_put(f.p[i], t);
        if (at + k > len) { CHECK(false, "piece longer than measured"); break; }
        memcpy(out.get() + at, t, k);
        at += k;
    }
    CHECK(at == len, "piece shorter than measured");
    return std::string(reinterpret_cast<const char*>(out.get()), at);
}

// whole, and cut at every position into two pieces
static void check_field(const std::string& s) {
    const Exact f(s);
    for (int as_line = 0; as_line < 2; ++as_line) {
        const std::string want = as_line ? host_line(s) : host_text(s);
        const std::string whole = piece(f, as_line, 0, f.n);
        CHECK(whole == want, "%s of %s: %s, host %s", as_line ? "input_line" : "matched_text", hex(s).c_str(), hex(whole).c_str(), hex(want).c_str());
        for (uint32_t c = 0; c <= f.n; ++c) {
            const std::string two = piece(f, as_line, 0, c) + piece(f, as_line, c, f.n);
            CHECK(two == want, "%s of %s cut at %u", as_line ? "input_line" : "matched_text", hex(s).c_str(), c);
        }
        // the sinks walk the same rules
        R::LenSink ls;
        if (as_line) ls.line(f.p.get(), f.n); else ls.text(f.p.get(), f.n);
        CHECK(ls.n == want.size(), "LenSink %llu, host %zu", (unsigned long long)ls.n, want.size());
        std::unique_ptr<uint8_t[]> out(new uint8_t[ls.n]);
        R::PutSink ps{out.get(), 0, ls.n};
        if (as_line) ps.line(f.p.get(), f.n); else ps.text(f.p.get(), f.n);
        CHECK(ps.pos == ls.n && std::string(reinterpret_cast<const char*>(out.get()), ls.n) == want, "PutSink of %s", hex(s).c_str());
    }
}

// the text of byte i does not change when bytes outside i-3 .. i+3 do
static void check_window(const std::string& s) {
    const Exact f(s);
    uint8_t t0[R::BYTE_TEXT_MAX], t1[R::BYTE_TEXT_MAX];
    for (uint32_t i = 0; i < f.n; ++i) {
        const uint32_t k0 = R::line_byte_put(f.p.get(), f.n, i, t0);
        for (uint8_t fill : {(uint8_t)'A', (uint8_t)0x80, (uint8_t)0xF0}) {
            std::string m = s;
            for (uint32_t j = 0; j < f.n; ++j) if (j + 3 < i || j > i + 3) m[j] = (char)fill;
            const Exact g(m);
            const uint32_t k1 = R::line_byte_put(g.p.get(), g.n, i, t1);
            CHECK(k0 == k1 && !memcmp(t0, t1, k0), "byte %u of %s depends on bytes outside its window", i, hex(s).c_str());
        }
    }
}

static const uint8_t ALPHABET[] = {0x00, 0x09, 0x1F, '"', 0x5C, 'A', 0x7F, 0x80, 0xBF, 0xC1, 0xC2, 0xE0, 0xA0, 0xED, 0x9F, 0xF0, 0x90, 0xF4, 0x8F, 0xF5, 0xFF};
constexpr size_t NA = sizeof(ALPHABET);

static void test_escape() {
    size_t count = 0;
    check_field("");
    for (size_t len = 1; len <= 3; ++len) {
        size_t total = 1;
        for (size_t k = 0; k < len; ++k) total *= NA;
        for (size_t v = 0; v < total; ++v) {
            std::string s;
            for (size_t k = 0, w = v; k < len; ++k, w /= NA) s.push_back((char)ALPHABET[w % NA]);
            check_field(s);
            check_window(s);
            ++count;
        }
    }
    for (int c = 0; c < 256; ++c) { check_field(std::string(1, (char)c)); ++count; }
    // the short escapes by name
    CHECK(piece(Exact(std::string("\b\f\n\r\t\"\\\x01\x1f", 9)), false, 0, 9) == "\\b\\f\\n\\r\\t\\\"\\\\\\u0001\\u001f", "short forms");
    printf("escape strings=%zu\n", count);
}

static std::string random_string(std::mt19937& rng) {
    const size_t n = 1 + rng() % 200;
    std::string s;
    for (size_t k = 0; k < n; ++k) s.push_back(rng() % 4 ? (char)ALPHABET[rng() % NA] : (char)(rng() & 0xFF));
    return s;
}
static void test_random() {
    std::mt19937 rng(20240607);
    for (int k = 0; k < 10000; ++k) check_field(random_string(rng));
    printf("random strings=10000\n");
}
static void test_window() {
    std::mt19937 rng(977);
    for (int k = 0; k < 2000; ++k) check_window(random_string(rng));
    printf("window strings=2000\n");
}

// <Ipv6Addr as Display> written with snprintf, as netaddr.h had it before its formatters could run on the device
static std::string model_ipv6(const uint16_t seg[8]) {
    char b[32];
    if (!seg[0] && !seg[1] && !seg[2] && !seg[3] && !seg[4] && seg[5] == 0xffff) {
        snprintf(b, sizeof(b), "::ffff:%u.%u.%u.%u", seg[6] >> 8, seg[6] & 255, seg[7] >> 8, seg[7] & 255);
        return b;
    }
    int bs = 0, bl = 0, cs = 0, cl = 0;
    for (int i = 0; i < 8; ++i) {
        if (seg[i] == 0) { if (cl == 0) cs = i; ++cl; if (cl > bl) { bl = cl; bs = cs; } }
        else cl = 0;
    }
    auto sub = [&](int lo, int hi) {
        std::string r;
        for (int i = lo; i < hi; ++i) { if (i > lo) r.push_back(':'); snprintf(b, sizeof(b), "%x", seg[i]); r += b; }
        return r;
    };
    if (bl > 1) return sub(0, bs) + "::" + sub(bs + bl, 8);
    return sub(0, 8);
}
static std::string full_ipv6(const uint16_t seg[8], bool pad) {   // all eight groups written out
    std::string r;
    char b[8];
    for (int i = 0; i < 8; ++i) { if (i) r.push_back(':'); snprintf(b, sizeof(b), pad ? "%04X" : "%x", seg[i]); r += b; }
    return r;
}
// the "cidr" value of a record for hit text T through render_core.h (with its quotes), in a block of exactly the measured length
static std::string core_cidr(const std::string& text, unsigned prefix) {
    const Exact f(text);
    R::LenSink ls;
    R::cidr_emit(f.p.get(), f.n, prefix, ls);
    std::unique_ptr<uint8_t[]> out(new uint8_t[ls.n]);
    R::PutSink ps{out.get(), 0, ls.n};
    R::cidr_emit(f.p.get(), f.n, prefix, ps);
    CHECK(ps.pos == ls.n, "cidr of %s: measured %llu, wrote %llu", text.c_str(), (unsigned long long)ls.n, (unsigned long long)ps.pos);
    return std::string(reinterpret_cast<const char*>(out.get()), ls.n);
}
static void check_v6(const uint16_t seg[8], const std::string& text, unsigned prefix) {
    IpAddr ip;
    CHECK(parse_ip(text.data(), text.size(), ip) && ip.v6, "%s does not parse", text.c_str());
    uint16_t m[8];
    for (int i = 0; i < 8; ++i) {
        const int left = (int)prefix - 16 * i;
        m[i] = left >= 16 ? seg[i] : left <= 0 ? 0 : (uint16_t)(seg[i] & (0xFFFF << (16 - left)));
    }
    const std::string want = "\"" + model_ipv6(m) + "/" + std::to_string(prefix) + "\"";
    CHECK("\"" + format_cidr(ip, prefix) + "\"" == want, "format_cidr(%s, %u) = %s, model %s", text.c_str(), prefix, format_cidr(ip, prefix).c_str(), want.c_str());
    const std::string got = core_cidr(text, prefix);
    CHECK(got == want, "cidr of %s/%u: %s, model %s", text.c_str(), prefix, got.c_str(), want.c_str());
}
static void test_ip() {
    size_t n = 0;
    // every position and length of a zero run in eight groups, in full, padded and compressed spelling
    for (int at = 0; at < 8; ++at)
        for (int len = 1; at + len <= 8; ++len) {
            uint16_t seg[8];
            for (int i = 0; i < 8; ++i) seg[i] = (i >= at && i < at + len) ? 0 : (uint16_t)(0x1a0 + i);
            check_v6(seg, full_ipv6(seg, false), 128);
            check_v6(seg, full_ipv6(seg, true), 128);
            check_v6(seg, model_ipv6(seg), 128);   // "::" forms parse back
            n += 3;
        }
    const uint16_t two_runs[8] = {1, 0, 0, 2, 3, 0, 0, 4}, longer_second[8] = {1, 0, 0, 2, 0, 0, 0, 4}, single[8] = {1, 2, 3, 0, 5, 6, 7, 8};
    const uint16_t zero[8] = {0}, mapped[8] = {0, 0, 0, 0, 0, 0xffff, 0x0102, 0x0304}, lead0[8] = {0x0001, 0x00a0, 0x0b00, 0xc000, 0x000d, 0x00e0, 0x0f00, 0x0abc};
    check_v6(two_runs, "1:0:0:2:3:0:0:4", 128);
    CHECK(core_cidr("1:0:0:2:3:0:0:4", 128) == "\"1::2:3:0:0:4/128\"", "the first of two equal runs wins");
    check_v6(longer_second, "1:0:0:2:0:0:0:4", 128);
    CHECK(core_cidr("1:0:0:2:0:0:0:4", 128) == "\"1:0:0:2::4/128\"", "the longer run wins");
    check_v6(single, "1:2:3:0:5:6:7:8", 128);
    CHECK(core_cidr("1:2:3:0:5:6:7:8", 128) == "\"1:2:3:0:5:6:7:8/128\"", "a single zero group is not compressed");
    check_v6(zero, "::", 128);
    CHECK(core_cidr("::", 0) == "\"::/0\"", "::");
    check_v6(mapped, "::ffff:1.2.3.4", 128);
    CHECK(core_cidr("::ffff:1.2.3.4", 128) == "\"::ffff:1.2.3.4/128\"", "mapped");
    check_v6(mapped, "::FFFF:102:304", 128);
    check_v6(lead0, full_ipv6(lead0, true), 128);
    CHECK(core_cidr(full_ipv6(lead0, true), 128) == "\"1:a0:b00:c000:d:e0:f00:abc/128\"", "leading zeros");
    const uint16_t embedded[8] = {0x2001, 0xdb8, 0, 0, 0, 0, 0xc000, 0x0280};
    check_v6(embedded, "2001:db8::192.0.2.128", 128);
    const uint16_t ones[8] = {0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff, 0xffff};
    const uint16_t mixed[8] = {0x2001, 0x0db8, 0x85a3, 0x0001, 0x8000, 0x8a2e, 0x0370, 0x7334};
    for (unsigned p = 0; p <= 128; ++p) {
        check_v6(ones, full_ipv6(ones, false), p);
        check_v6(mixed, full_ipv6(mixed, false), p);
        check_v6(mapped, "::ffff:1.2.3.4", p);
        n += 3;
    }
    for (unsigned p = 0; p <= 32; ++p)
        for (const char* t : {"255.255.255.255", "10.200.3.77", "1.2.3.4"}) {
            unsigned a[4];
            sscanf(t, "%u.%u.%u.%u", &a[0], &a[1], &a[2], &a[3]);
            const uint32_t v = (a[0] << 24) | (a[1] << 16) | (a[2] << 8) | a[3], m = p ? v & (0xFFFFFFFFu << (32 - p)) : 0;
            char b[40];
            snprintf(b, sizeof(b), "\"%u.%u.%u.%u/%u\"", m >> 24, (m >> 16) & 255, (m >> 8) & 255, m & 255, p);
            CHECK(core_cidr(t, p) == b, "cidr of %s/%u: %s", t, p, core_cidr(t, p).c_str());
            ++n;
        }
    // texts that do not parse: json_escape(T + "/" + P)
    for (const std::string& t : {std::string("1::2::3"), std::string("12345::1"), std::string("1.2.3.04"), std::string("fe80::1%eth\"0"), std::string(""), std::string("a\tb\x80")}) {
        IpAddr ip;
        CHECK(!parse_ip(t.data(), t.size(), ip), "%s parses", t.c_str());
        std::string want;
        json_escape(t + "/" + std::to_string(77), want);
        CHECK(core_cidr(t, 77) == want, "fallback cidr of %s: %s", t.c_str(), core_cidr(t, 77).c_str());
        ++n;
    }
    printf("ip cases=%zu\n", n);
}

static void test_decimal() {
    for (uint64_t v : {0ull, 9ull, 10ull, 99ull, 100ull, 4294967295ull, 4294967296ull, 18446744073709551615ull, 9999999999999999999ull, 10000000000000000000ull}) {
        char want[32];
        const int k = snprintf(want, sizeof(want), "%llu", (unsigned long long)v);
        std::unique_ptr<uint8_t[]> out(new uint8_t[R::dec_len(v)]);
        CHECK((int)R::dec_len(v) == k && (int)R::dec_put(v, out.get()) == k && !memcmp(out.get(), want, k), "decimal %s", want);
    }
    printf("decimal ok\n");
}

// whole records against a std::string assembly in the manner of matchy_scan_hit_to_json
struct MapPayloads {
    const std::map<uint32_t, std::string>& json;
    const std::vector<int64_t>& data_offsets;
    template <class S> void one(S& s, uint32_t off) { const std::string& j = json.at(off); s.bytes(reinterpret_cast<const uint8_t*>(j.data()), (uint32_t)j.size()); }
    template <class S> void array(S& s, uint32_t first, uint32_t n) {
        bool any = false;
        for (uint32_t k = 0; k < n; ++k) {
            if (data_offsets[first + k] < 0) continue;
            if (any) MXY_RC_LIT(s, ","); else MXY_RC_LIT(s, "\"data\":[");
            one(s, (uint32_t)data_offsets[first + k]);
            any = true;
        }
        if (any) MXY_RC_LIT(s, "],");
    }
};
static void test_records() {
    const std::map<uint32_t, std::string> json = {{8, "{\"a\":\"x\\\"y\"}"}, {40, "null"}, {99, "[1,2.5,{\"k\":{}}]"}};
    const std::vector<int64_t> offs = {8, -1, 99, -1, -1, 40};
    struct Case { uint8_t kind; std::string hit, line; uint32_t value, n_ids; uint8_t prefix; std::string source; uint64_t number; };
    const std::vector<Case> cases = {
        {2, "10.1.2.3", "from 10.1.2.3 \"q\"\r", 8, 0, 24, "a \"b\".log", 0},
        {2, "2001:db8::1", "x 2001:db8::1 \xff\xe0\xa0", 40, 0, 33, "-", (1ull << 40) + 5},
        {2, "1::2::3", "1::2::3", 99, 0, 128, "s", 18446744073709551614ull},
        {3, "evil\"\\.example", "\tGET evil\"\\.example \xf0\x90", 0, 3, 0, "p\\q", 7},
        {3, "none.example", "", 3, 2, 0, "-", 1},
        {3, "one.example", "one.example", 5, 1, 0, "-", 4294967295ull},
        {3, "zero", "zero", 0, 0, 0, "-", 2},
    };
    size_t n = 0;
    for (const Case& c : cases)
        for (uint32_t flags : {0u, R::FLAG_LINE_NUMBERS, R::FLAG_LINE_NUMBERS | R::FLAG_INPUT_LINE, R::FLAG_INPUT_LINE}) {
            std::string src, want = "{";
            json_escape(c.source, src);
            std::string lines;
            if (flags & R::FLAG_INPUT_LINE) { lines += "\"input_line\":"; std::string l; utf8_lossy_append((const uint8_t*)c.line.data(), c.line.size(), l); json_escape(l, lines); lines += ","; }
            if (flags) lines += "\"line_number\":" + std::to_string(c.number) + ",";
            if (c.kind == 2) {
                IpAddr ip;
                std::string cidr = parse_ip(c.hit.data(), c.hit.size(), ip) ? format_cidr(ip, c.prefix) : c.hit + "/" + std::to_string(c.prefix);
                want += "\"cidr\":"; json_escape(cidr, want);
                want += ",\"data\":" + json.at(c.value) + "," + lines + "\"match_type\":\"ip\",\"matched_text\":"; json_escape(c.hit, want);
                want += ",\"prefix_len\":" + std::to_string(c.prefix);
            } else {
                std::string arr;
                for (uint32_t k = 0; k < c.n_ids; ++k) if (offs[c.value + k] >= 0) { if (!arr.empty()) arr += ","; arr += json.at((uint32_t)offs[c.value + k]); }
                if (!arr.empty()) want += "\"data\":[" + arr + "],";
                want += lines + "\"match_type\":\"pattern\",\"matched_text\":"; json_escape(c.hit, want);
                want += ",\"pattern_count\":" + std::to_string(c.n_ids);
            }
            want += ",\"source\":" + src + ",\"timestamp\":\"0.000\"}\n";
            const Exact hit(c.hit), line(c.line), source(src);
            R::RecordIn r{hit.p.get(), hit.n, c.value, c.n_ids, c.kind, c.prefix, flags, line.p.get(), line.n, c.number, source.p.get(), source.n};
            MapPayloads pay{json, offs};
            R::LenSink ls;
            R::record_emit(r, pay, ls);
            CHECK(ls.n == want.size(), "record length %llu, host %zu: %s", (unsigned long long)ls.n, want.size(), want.c_str());
            // exact block; then a block one byte short, which must hold the same bytes in front of its end while pos counts on
            for (uint64_t cap : {ls.n, ls.n ? ls.n - 1 : 0, (uint64_t)0}) {
                std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
                R::PutSink ps{out.get(), 0, cap};
                R::record_emit(r, pay, ps);
                CHECK(ps.pos == ls.n && !memcmp(out.get(), want.data(), cap < want.size() ? cap : want.size()), "record text at capacity %llu: %s", (unsigned long long)cap, want.c_str());
            }
            ++n;
        }
    printf("records=%zu\n", n);
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "all";
    const bool all = what == "all";
    if (all || what == "escape") test_escape();
    if (all || what == "window") test_window();
    if (all || what == "random") test_random();
    if (all || what == "ip") test_ip();
    if (all || what == "decimal") test_decimal();
    if (all || what == "records") test_records();
    if (failures) { printf("render_core FAILED: %d\n", failures); return 1; }
    printf("render_core ok\n");
    return 0;
}
