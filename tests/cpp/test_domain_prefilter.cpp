// CPU check of the label-window rule of k_anchor's domain drain (matchy_amd/csrc/domain_prefilter.h) and of the exact table of
// long-label prefixes k_validate_dom asks (hashes.h: tld_pfx_*), against the shipped public-suffix list:
//  (a) label_window_keep() keeps every last label of the list: every length, every alignment of the window in the dwords it is cut
//      from, every boundary byte behind the labels of 7 bytes or fewer;
//  (b) the table holds the first 8 bytes of every last label of 8 bytes or more and nothing else (random 8-byte keys);
//  (c) label_window_keep() against a byte-by-byte restatement of val_domain's first steps (validate_kernels.hip) over random and
//      constructed windows: it never drops what the restatement accepts, and it drops every window with a dot in the label or a
//      non-boundary byte behind it — what it keeps beyond the restatement is what the Bloom filter lets through;
//  (d) over log files given as NAME=PATH: the survivors of the rule and of the rule it replaced (look 16 bytes further for a dot), by
//      label length. The caller asserts on the printed counts.
// Build: g++ -O2 -std=c++17 -I matchy_amd/csrc tests/cpp/test_domain_prefilter.cpp -o /tmp/test_domain_prefilter
// Run:   /tmp/test_domain_prefilter matchy_amd/data/psl.bin [NAME=LOG ...]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <unordered_set>
#include <vector>

#include "domain_prefilter.h"

using namespace mxy;

#define FAIL(...) do { printf("FAIL: " __VA_ARGS__); printf("\n"); return 1; } while (0)

struct Slot { uint32_t x, y; };

// the byte classes as the extractor defines them (boundary set, domain characters)
static bool is_boundary(unsigned b) {
    static const unsigned char cs[] = {0x09, 0x0a, 0x0d, 0x20, 0x22, 0x27, 0x28, 0x29, 0x2c, 0x2f, 0x3a, 0x3b, 0x3c, 0x3d, 0x3e, 0x40, 0x5b, 0x5d, 0x7b, 0x7d};
    for (unsigned char c : cs) if (c == b) return true;
    return false;
}
static bool is_digit(unsigned b) { return b >= '0' && b <= '9'; }
static bool is_alpha(unsigned b) { return (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'); }
static bool is_ld(unsigned b) { return is_digit(b) || is_alpha(b) || b >= 0x80; }
static bool is_dc(unsigned b) { return is_ld(b) || b == '.' || b == '-'; }
static bool is_tl(unsigned b) { return (b >= 'a' && b <= 'z') || b >= 0x80; }   // first byte of a last label of the shipped list

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

// ---- the list
static std::vector<std::string> g_labels;                    // distinct last labels
static std::unordered_set<std::string> g_short;              // those of <= 7 bytes
static std::unordered_set<std::string> g_windows;            // first 8 bytes of those of >= 8 bytes
static std::vector<uint32_t> g_filter(TLD_PREFILTER_BITS / 32, 0), g_filter_old(TLD_PREFILTER_BITS / 32, 0);
static std::vector<Slot> g_pfx(1u << TLD_PFX_BITS, Slot{0, 0});

static bool load_list(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> buf;
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    if (buf.size() < 16 || memcmp(buf.data(), "PSLB", 4) != 0) return false;
    uint32_t count;
    memcpy(&count, &buf[8], 4);
    std::string prev;
    std::set<std::string> labels;
    size_t p = 16;
    for (uint32_t i = 0; i < count; ++i) {   // front-coded: shared prefix length, rest length, rest
        if (p + 2 > buf.size()) return false;
        const uint8_t shared = buf[p], rest = buf[p + 1];
        p += 2;
        if (shared > prev.size() || p + rest > buf.size()) return false;
        std::string s = prev.substr(0, shared) + std::string((const char*)&buf[p], rest);
        p += rest;
        const size_t dot = s.rfind('.');
        const std::string l = dot == std::string::npos ? s : s.substr(dot + 1);
        if (!l.empty()) labels.insert(l);
        prev.swap(s);
    }
    g_labels.assign(labels.begin(), labels.end());
    return true;
}

static bool in_filter(const std::vector<uint32_t>& flt, const uint8_t* key, size_t n) {
    uint8_t k8[8] = {0};
    memcpy(k8, key, n);
    uint32_t lo, hi;
    memcpy(&lo, k8, 4); memcpy(&hi, k8 + 4, 4);
    const uint32_t h8 = tld_hash8(lo, hi);
    const uint32_t b1 = h8 & (TLD_PREFILTER_BITS - 1), b2 = (h8 >> 14) & (TLD_PREFILTER_BITS - 1);
    return (flt[b1 >> 5] >> (b1 & 31)) & (flt[b2 >> 5] >> (b2 & 31)) & 1u;
}

static bool keep_window(const uint8_t* w) {
    uint32_t lo, hi;
    memcpy(&lo, w, 4); memcpy(&hi, w + 4, 4);
    return label_window_keep(lo, hi, g_filter.data(), [](uint32_t b) { return is_boundary(b); });
}

// the window as the drain gets it: two dwords cut out of three aligned ones at byte offset sh (raw_read, k_anchor.hip)
static bool keep_window_cut(const uint8_t* w, uint32_t sh, uint32_t r) {
    uint8_t b[12];
    for (int i = 0; i < 12; ++i) b[i] = (uint8_t)(r >> (i % 4 * 8 + i / 4));   // what lies around the window: anything
    memcpy(b + sh, w, 8);
    uint32_t q[3];
    memcpy(q, b, 12);
    const uint64_t a = (uint64_t)q[0] | ((uint64_t)q[1] << 32), c = (uint64_t)q[1] | ((uint64_t)q[2] << 32);
    const uint32_t lo = (uint32_t)(a >> (8 * sh)), hi = (uint32_t)(c >> (8 * sh));
    return label_window_keep(lo, hi, g_filter.data(), [](uint32_t x) { return is_boundary(x); });
}

// ---- val_domain's first steps, byte by byte, as far as 8 bytes show them. 0: a dot in the label (a later dot owns the run) or a
// non-boundary byte behind it; 1: the label can be no suffix's last label; 2: it can (exactly, from the list).
static int restated(const uint8_t* w) {
    size_t ll = 0;
    while (ll < 8 && is_dc(w[ll])) {
        if (w[ll] == '.') return 0;
        ++ll;
    }
    if (ll < 8) {
        if (!is_boundary(w[ll])) return 0;
        return g_short.count(std::string((const char*)w, ll)) ? 2 : 1;
    }
    return g_windows.count(std::string((const char*)w, 8)) ? 2 : 1;
}

// ---- the rule this one replaced: labels that end inside the window as above with a filter of the labels of <= 8 bytes; a window full of
// domain characters looks 16 bytes further for a dot in front of the first non-domain byte and keeps the anchor if there is none
static bool old_rule(const uint8_t* w24) {
    size_t ll = 0;
    while (ll < 24 && is_dc(w24[ll])) {
        if (w24[ll] == '.') return false;
        ++ll;
    }
    if (ll >= 8) return true;
    return is_boundary(w24[ll]) && in_filter(g_filter_old, w24, ll);
}

enum Cls { LETTER, DIGIT, DASH, DOT, BOUND, OTHER, HIGH, NCLS };
static uint8_t pick(int cls, uint32_t r) {
    static const char letters[] = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
    static const unsigned char bounds[] = {0x09, 0x0a, 0x0d, 0x20, 0x22, 0x27, 0x28, 0x29, 0x2c, 0x2f, 0x3a, 0x3b, 0x3c, 0x3d, 0x3e, 0x40, 0x5b, 0x5d, 0x7b, 0x7d};
    static const unsigned char others[] = {'_', '%', '+', '~', '!', '#', '&', '*', '?', '\\', '^', '`', '|', 0x00, 0x1F, 0x7F, '$'};
    switch (cls) {
        case LETTER: return (uint8_t)letters[r % 52];
        case DIGIT: return (uint8_t)('0' + r % 10);
        case DASH: return '-';
        case DOT: return '.';
        case BOUND: return bounds[r % sizeof bounds];
        case OTHER: return others[r % sizeof others];
        default: return (uint8_t)(0x80 + r % 128);
    }
}

static long g_cases = 0, g_verdict[3] = {0, 0, 0}, g_extra = 0, g_undecided = 0, g_bad = 0;
static void check(const uint8_t* w) {
    const int ref = restated(w);
    const bool keep = keep_window(w);
    ++g_cases;
    ++g_verdict[ref];
    const bool ok = ref == 2 ? keep : ref == 0 ? !keep : true;
    if (ref == 1) { ++g_undecided; g_extra += keep; }
    if (!ok && g_bad++ < 10) {
        printf("MISMATCH restated %d keep %d window", ref, (int)keep);
        for (int i = 0; i < 8; ++i) printf(" %02x", w[i]);
        printf("\n");
    }
}

int main(int argc, char** argv) {
    if (argc < 2 || !load_list(argv[1])) FAIL("usage: test_domain_prefilter psl.bin [NAME=LOG ...]");
    size_t n_short8 = 0, n_long = 0, n_new = 0;
    for (const std::string& l : g_labels) {
        n_new += prefilter_add_label(g_filter.data(), g_pfx.data(), (const uint8_t*)l.data(), l.size());
        if (l.size() <= 8) ++n_short8;
        else ++n_long;
        if (l.size() <= 7) g_short.insert(l);
        else g_windows.insert(l.substr(0, 8));
        if (l.size() <= 8) {   // the filter as it was: labels that fit the window
            uint8_t k8[8] = {0};
            memcpy(k8, l.data(), l.size());
            uint32_t lo, hi;
            memcpy(&lo, k8, 4); memcpy(&hi, k8 + 4, 4);
            const uint32_t h8 = tld_hash8(lo, hi);
            const uint32_t b1 = h8 & (TLD_PREFILTER_BITS - 1), b2 = (h8 >> 14) & (TLD_PREFILTER_BITS - 1);
            g_filter_old[b1 >> 5] |= 1u << (b1 & 31);
            g_filter_old[b2 >> 5] |= 1u << (b2 & 31);
        }
    }
    std::unordered_set<std::string> long_windows;
    for (const std::string& l : g_labels) if (l.size() > 8) long_windows.insert(l.substr(0, 8));
    auto density = [](const std::vector<uint32_t>& f) { size_t n = 0; for (uint32_t w : f) n += (size_t)__builtin_popcount(w); return 100.0 * (double)n / (double)(f.size() * 32); };
    printf("list: %zu last labels, %zu of 8 bytes or fewer, %zu longer with %zu distinct 8-byte prefixes; table keys %zu; filter density %.1f %% -> %.1f %%\n",
           g_labels.size(), n_short8, n_long, long_windows.size(), n_new, density(g_filter_old), density(g_filter));
    if (g_labels.size() < 1000 || n_long < 100) FAIL("the list is not the shipped one");

    // ---- (a) every last label of the list is kept
    {
        static const unsigned char bounds[] = {0x09, 0x0a, 0x0d, 0x20, 0x22, 0x27, 0x28, 0x29, 0x2c, 0x2f, 0x3a, 0x3b, 0x3c, 0x3d, 0x3e, 0x40, 0x5b, 0x5d, 0x7b, 0x7d};
        long n = 0, lens[64] = {0};
        for (const std::string& l : g_labels) {
            ++lens[std::min<size_t>(l.size(), 63)];
            uint8_t w[8];
            if (l.size() >= 8) {
                memcpy(w, l.data(), 8);
                for (uint32_t sh = 0; sh < 4; ++sh, ++n)
                    if (!keep_window_cut(w, sh, rnd())) FAIL("label %s (%zu bytes) dropped at alignment %u", l.c_str(), l.size(), sh);
                continue;
            }
            for (unsigned char stop : bounds)
                for (int fill = 0; fill < 4; ++fill) {
                    memcpy(w, l.data(), l.size());
                    w[l.size()] = stop;
                    // behind the boundary: letters, dots, boundaries, anything
                    for (size_t k = l.size() + 1; k < 8; ++k) w[k] = fill == 0 ? 'a' : fill == 1 ? '.' : fill == 2 ? ' ' : (uint8_t)rnd();
                    for (uint32_t sh = 0; sh < 4; ++sh, ++n)
                        if (!keep_window_cut(w, sh, rnd())) FAIL("label %s dropped: stop byte 0x%02x, fill %d, alignment %u", l.c_str(), stop, fill, sh);
                }
        }
        printf("(a) %ld windows of %zu labels kept; labels by length:", n, g_labels.size());
        for (int k = 1; k < 64; ++k) if (lens[k]) printf(" %d:%ld", k, lens[k]);
        printf("\n");
        for (int k = 2; k <= 12; ++k) if (!lens[k]) FAIL("the list has no last label of %d bytes", k);
    }

    // ---- (b) the exact table: the windows of the labels of 8 bytes or more, nothing else
    {
        size_t used = 0;
        for (const Slot& s : g_pfx) used += (s.x | s.y) != 0;
        if (used != g_windows.size() || n_new != g_windows.size()) FAIL("table holds %zu keys (%zu entered), the list has %zu windows", used, n_new, g_windows.size());
        if (used > TLD_PFX_MAX_KEYS) FAIL("table over its limit");
        for (const std::string& w : g_windows) {
            uint32_t lo, hi;
            memcpy(&lo, w.data(), 4); memcpy(&hi, w.data() + 4, 4);
            if (!tld_pfx_has(g_pfx.data(), lo, hi)) FAIL("window %s is not in the table", w.c_str());
        }
        for (const std::string& w : long_windows) if (!g_windows.count(w)) FAIL("prefix %s missing", w.c_str());
        long hits = 0;
        const long N = 4000000;
        for (long i = 0; i < N; ++i) {
            uint8_t k[8];
            const uint32_t a = rnd(), b = rnd();
            if (i & 1) for (int q = 0; q < 8; ++q) k[q] = (uint8_t)('a' + ((q < 4 ? a : b) >> (8 * (q & 3))) % 26);   // letters only
            else { memcpy(k, &a, 4); memcpy(k + 4, &b, 4); }
            if (i % 7 == 0) {   // a listed window with one byte changed
                auto it = g_windows.begin();
                std::advance(it, (long)(a % g_windows.size()) % 16);
                memcpy(k, it->data(), 8);
                if (i % 21) k[b % 8] ^= (uint8_t)(1u << (b >> 8) % 7);   // ... or as it is
            }
            uint32_t lo, hi;
            memcpy(&lo, k, 4); memcpy(&hi, k + 4, 4);
            const bool want = g_windows.count(std::string((const char*)k, 8)) != 0, got = (lo | hi) != 0 && tld_pfx_has(g_pfx.data(), lo, hi);
            hits += want;
            if (want != got) FAIL("table says %d for a key the list %s", (int)got, want ? "has" : "does not have");
        }
        printf("(b) table: %zu keys = the list's windows (%zu from labels of 9 bytes or more); %ld random keys, %ld of them listed\n", used, long_windows.size(), N, hits);
    }

    // ---- (c) against the restatement
    {
        // labels of 1..12 bytes of letters, digits, dashes and high bytes, every stop byte behind them, then anything
        for (uint32_t len = 1; len <= 12; ++len)
            for (uint32_t stop = 0; stop < 256; ++stop)
                for (int rep = 0; rep < 60; ++rep) {
                    uint8_t w[16];
                    const uint32_t r = rnd();
                    for (uint32_t k = 0; k < len; ++k) { const uint32_t q = rnd(); w[k] = pick(q % 16 < 11 ? LETTER : q % 16 < 13 ? DIGIT : q % 16 < 14 ? DASH : HIGH, q >> 4); }
                    w[len] = (uint8_t)stop;
                    for (uint32_t k = len + 1; k < 16; ++k) w[k] = pick((int)((r >> (2 * k)) % NCLS), rnd());
                    check(w);
                }
        // listed labels (whole, cut short, one byte changed) with every stop byte; a dot, a dash or a high byte at every position
        for (size_t li = 0; li < g_labels.size(); ++li) {
            const std::string& l = g_labels[li];
            for (uint32_t stop = 0; stop < 256; ++stop) {
                uint8_t w[80];
                memset(w, ' ', sizeof w);
                memcpy(w, l.data(), l.size());
                w[l.size()] = (uint8_t)stop;
                check(w);
                if (stop < 8) {
                    for (int cls : {DOT, DASH, HIGH, OTHER, BOUND}) { uint8_t v[80]; memcpy(v, w, 80); v[stop] = pick(cls, rnd()); check(v); }
                    uint8_t v[80];
                    memcpy(v, w, 80);
                    v[stop] ^= 0x01;
                    check(v);
                }
                if (stop >= 1 && stop < l.size() && stop <= 8) {   // the label cut after `stop` bytes by a boundary
                    uint8_t v[80];
                    memcpy(v, w, 80);
                    v[stop] = pick(BOUND, rnd());
                    check(v);
                }
            }
        }
        // random windows: all byte values; the seven classes evenly; letters with a few other bytes
        for (long i = 0; i < 3000000; ++i) {
            uint8_t w[8];
            const int mode = (int)(i % 3);
            for (int k = 0; k < 8; ++k) {
                const uint32_t r = rnd();
                w[k] = mode == 0 ? (uint8_t)r : mode == 1 ? pick((int)(r % NCLS), r >> 3) : pick(r % 32 < 27 ? LETTER : (int)(r % NCLS), r >> 5);
            }
            check(w);
        }
        printf("(c) %ld windows: restated verdicts drop %ld / not listed %ld / listed %ld; kept beyond the list %ld of %ld = %.2f %%; mismatches %ld\n",
               g_cases, g_verdict[0], g_verdict[1], g_verdict[2], g_extra, g_undecided, 100.0 * (double)g_extra / (double)std::max(1L, g_undecided), g_bad);
        if (g_bad) return 1;
        if (g_cases < 3000000 || g_verdict[0] < 100000 || g_verdict[1] < 100000 || g_verdict[2] < 100000) FAIL("the inputs do not cover the verdicts");
        // two probes into a filter of density d pass d^2 of the keys that are not in it: 3.1 % at the 17.5 % of the shipped list
        const double d = density(g_filter) / 100.0;
        if ((double)g_extra > (d * d + 0.005) * (double)g_undecided) FAIL("the rule keeps more than the filter's rate beyond the list");
    }

    // ---- (d) survivors over log files
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) continue;
        const std::string name(argv[i], eq - argv[i]);
        FILE* f = fopen(eq + 1, "rb");
        if (!f) FAIL("cannot open %s", eq + 1);
        std::vector<uint8_t> log;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) log.insert(log.end(), tmp, tmp + n);
        fclose(f);
        log.insert(log.end(), 32, ' ');   // positions past the end are staged as ' '
        long anchors = 0, short_n = 0, short_old = 0, short_new = 0, short_diff = 0, long_n = 0, long_old = 0, long_new = 0, long_listed = 0;
        for (size_t j = 2; j + 32 <= log.size(); ++j) {
            if (log[j - 1] != '.' || !is_ld(log[j - 2]) || !is_tl(log[j])) continue;   // label byte, '.', byte that can start a last label
            ++anchors;
            const uint8_t* w = &log[j];
            size_t ll = 0;
            while (ll < 8 && is_dc(w[ll]) && w[ll] != '.') ++ll;
            const bool o = old_rule(w), k = keep_window(w);
            if (ll < 8) { ++short_n; short_old += o; short_new += k; short_diff += o != k; }
            else { ++long_n; long_old += o; long_new += k; long_listed += restated(w) == 2; }
        }
        printf("%s: domain anchors %ld; short labels %ld survivors old %ld new %ld differing %ld; long labels %ld survivors old %ld new %ld listed %ld\n",
               name.c_str(), anchors, short_n, short_old, short_new, short_diff, long_n, long_old, long_new, long_listed);
    }
    printf("domain_prefilter ok\n");
    return 0;
}
