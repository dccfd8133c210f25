// CPU check of the bit-sliced label rules of k_validate_dom (matchy_amd/csrc/domain_planes.h):
//  (a) context_planes(): every byte value at every one of the 32 context positions against the byte-wise class definitions;
//  (b) domain_rules() against two references — the byte-lane SWAR function it replaced (val_domain_pre, kept here verbatim with host
//      shims for the device intrinsics) and a plain byte loop written from the rules — on constructed and random contexts: verdict,
//      start and end must be equal in every case, and every verdict must occur often enough that the inputs mean something.
// Build: g++ -O2 -std=c++17 -I matchy_amd/csrc tests/cpp/test_domain_planes.cpp -o /tmp/test_domain_planes
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "domain_planes.h"

using namespace mxy;

// ---- host shims for the device code below
#define __device__
#define __forceinline__ inline
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline int __ffsll(long long x) { return __builtin_ffsll(x); }
static inline int __clzll(long long x) { return __builtin_clzll((unsigned long long)x); }   // callers never pass 0
static inline int __popcll(uint64_t x) { return __builtin_popcountll(x); }
using std::min;

// the byte classes as the extractor defines them (matchy-extractor/src/lib.rs:1568-1593 boundary set, :1597-1629 domain chars)
static bool is_boundary(unsigned b) {
    static const unsigned char cs[] = {0x09, 0x0a, 0x0d, 0x20, 0x22, 0x27, 0x28, 0x29, 0x2c, 0x2f, 0x3a, 0x3b, 0x3c, 0x3d, 0x3e, 0x40, 0x5b, 0x5d, 0x7b, 0x7d};
    for (unsigned char c : cs) if (c == b) return true;
    return false;
}
static bool is_digit(unsigned b) { return b >= '0' && b <= '9'; }
static bool is_alpha(unsigned b) { return (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'); }
static bool is_dc(unsigned b) { return is_digit(b) || is_alpha(b) || b == '.' || b == '-' || b >= 0x80; }
static bool d_is_boundary(uint32_t b) { return is_boundary(b); }

// ---- reference 1: the SWAR form, verbatim from device_common.h / validate_kernels.hip as they stood before domain_planes.h
struct ByteMasks { uint64_t dc, dot, dash, high; };
struct ByteMasks32 { uint32_t dc, dot, dash, high; };
__device__ __forceinline__ ByteMasks32 domain_masks32(uint32_t x) {
    constexpr uint32_t H = 0x80808080u, L7 = 0x7F7F7F7Fu;
    const uint32_t t = x & L7, l = t | 0x20202020u;
    const uint32_t dig = (t + 0x50505050u) & ~(t + 0x46464646u);   // '0'..'9'
    const uint32_t alp = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u);   // 'a'..'z' after case folding
    const uint32_t ndot = (t ^ 0x2E2E2E2Eu) + L7, ndash = (t ^ 0x2D2D2D2Du) + L7;  // bit 7 set iff different
    ByteMasks32 m;
    m.high = x & H;
    m.dot = ~ndot & ~x & H;
    m.dash = ~ndash & ~x & H;
    m.dc = (((dig | alp) & ~x) | m.dot | m.dash | m.high) & H;  // DOMAIN_CHAR_LOOKUP (ext:1597-1629)
    return m;
}
__device__ __forceinline__ ByteMasks domain_masks(uint64_t x) {
    const ByteMasks32 lo = domain_masks32((uint32_t)x), hi = domain_masks32((uint32_t)(x >> 32));
    ByteMasks m;
    m.dc = (uint64_t)lo.dc | ((uint64_t)hi.dc << 32);
    m.dot = (uint64_t)lo.dot | ((uint64_t)hi.dot << 32);
    m.dash = (uint64_t)lo.dash | ((uint64_t)hi.dash << 32);
    m.high = (uint64_t)lo.high | ((uint64_t)hi.high << 32);
    return m;
}

// The same for an anchor that comes with its context record (k_anchor copies log[j-24, j+8) from its LDS window):
// w = log[j, j+8), b0 = log[j-8, j), b1 = log[j-16, j-8), b2 = log[j-24, j-16). The common case — last label of <= 7
// bytes that alone is a public suffix, name no longer than the context — is decided with mask arithmetic on these
// registers, without a per-byte loop and without divergent control flow (k_validate is bound by scalar-ALU issue, i.e.
// by control flow): the rules of is_valid_domain (ext:637-689) become tests on the dot / dash / domain-char masks.
// Everything else is left to the general path (val_domain, in k_validate).
// Returns 0 (no domain), 1 (domain: start / end set, the whole name lies in the context) or 2 (undecided: general path).
__device__ __forceinline__ int val_domain_pre(const uint2* tldtab, uint32_t min_labels, uint32_t j, uint2 w, uint64_t b0, uint64_t b1,
                                              uint64_t b2, uint32_t& start, uint32_t& end) {
    constexpr uint64_t H = 0x8080808080808080ull;
    const uint64_t w64 = (uint64_t)w.x | ((uint64_t)w.y << 32);
    const ByteMasks mw = domain_masks(w64);
    // last label = leading domain-char bytes of w; ll = its length (8: not terminated within the window)
    const uint64_t ndc = ~mw.dc & H;
    const uint32_t ll = ndc ? (uint32_t)(__ffsll((long long)ndc) - 1) >> 3 : 8u;
    if (ll <= 7 && ll >= 1) {
        const uint64_t below = (1ull << (8 * ll)) - 1ull;            // the label's bytes
        if (mw.dot & below) return 0;                                // a later dot owns this run
        const uint32_t stop_c = (uint32_t)(w64 >> (8 * ll)) & 0xFF;
        if (!d_is_boundary(stop_c)) return 0;
        const uint32_t lo = (uint32_t)(w64 & below), hi = (uint32_t)((w64 & below) >> 32);
        uint32_t slot = tld_tab_slot(lo, hi);
        bool alone = false;
        for (;;) {
            const uint2 t = tldtab[slot];
            if ((t.y >> 24) == 0) return 0;
            if (t.x == lo && (t.y & 0xFFFFFFu) == hi) { alone = (t.y >> 24) & 1; break; }
            slot = (slot + 1) & ((1u << TLD_TAB_BITS) - 1);
        }
        if (alone) {
            // the 24 bytes in front of the label, address order: b2 | b1 | b0; the run extends leftwards from the top
            // byte of b0 (the dot at j-1) while bytes are domain chars
            const ByteMasks m0 = domain_masks(b0), m1 = domain_masks(b1), m2 = domain_masks(b2);
            const uint64_t n0m = ~m0.dc & H, n1m = ~m1.dc & H, n2m = ~m2.dc & H;
            const uint32_t c0 = n0m ? (uint32_t)__clzll((long long)n0m) >> 3 : 8u;   // domain chars at the top of b0
            const uint32_t c1 = n1m ? (uint32_t)__clzll((long long)n1m) >> 3 : 8u, c2 = n2m ? (uint32_t)__clzll((long long)n2m) >> 3 : 8u;
            const uint32_t consumed = c0 < 8 ? c0 : (c1 < 8 ? 8 + c1 : 16 + c2);
            if (consumed < 24 || j == 24) {   // the run starts inside the context (or at the start of the buffer)
                // region masks: the top `k` bytes of each word that belong to the run
                auto top = [](uint32_t k) -> uint64_t { return k == 0 ? 0ull : (~0ull << (64 - 8 * k)); };
                const uint64_t r0 = top(min(consumed, 8u)), r1 = top(consumed > 8 ? min(consumed - 8, 8u) : 0u),
                               r2 = top(consumed > 16 ? consumed - 16 : 0u);
                // "byte to the right" (one position closer to the label) moved onto each byte: shift towards lower
                // addresses; the byte right of b0's top byte is the label's first byte (neither dot nor dash)
                const uint64_t d0 = m0.dot >> 8, d1 = (m1.dot >> 8) | (m0.dot << 56), d2 = (m2.dot >> 8) | (m1.dot << 56);
                const uint64_t s0 = m0.dash >> 8, s1 = (m1.dash >> 8) | (m0.dash << 56), s2 = (m2.dash >> 8) | (m1.dash << 56);
                // bad events: empty label (two dots in a row), label starting with '-' (dot, then dash to its right),
                // label ending with '-' (dash, then dot to its right)
                const uint64_t bad = ((m0.dot & (d0 | s0)) | (m0.dash & d0)) & r0;
                const uint64_t bad1 = ((m1.dot & (d1 | s1)) | (m1.dash & d1)) & r1, bad2 = ((m2.dot & (d2 | s2)) | (m2.dash & d2)) & r2;
                const uint32_t ndots = (uint32_t)(__popcll(m0.dot & r0) + __popcll(m1.dot & r1) + __popcll(m2.dot & r2));
                // leftmost byte of the run: must not be a dot (empty leftmost label) or a dash
                const uint32_t li = 24 - consumed;                       // its index in address order (consumed >= 1: the dot)
                const uint64_t lw = li < 8 ? b2 : li < 16 ? b1 : b0;
                const uint32_t left_c = (uint32_t)(lw >> (8 * (li & 7))) & 0xFF;
                const uint32_t fi = 23 - consumed;                       // byte in front of the run (if inside the context)
                const uint64_t fw = fi < 8 ? b2 : fi < 16 ? b1 : b0;
                const uint32_t first_c = consumed < 24 ? (uint32_t)(fw >> (8 * (fi & 7))) & 0xFF : 0x100u;
                const uint32_t lastc = (uint32_t)(w64 >> (8 * (ll - 1))) & 0xFF;
                const bool any_bad = (bad | bad1 | bad2) != 0 || lastc == '-' || consumed == 0 || left_c == '.' || left_c == '-';
                if (any_bad || ndots == 0 || 1 + ndots < min_labels) return 0;
                if (first_c != 0x100 && !d_is_boundary(first_c)) return 0;
                const uint32_t s_pos = j - consumed;
                const bool high = ((m0.high & r0) | (m1.high & r1) | (m2.high & r2) | (mw.high & below)) != 0;
                if (high) return 2;   // needs the UTF-8 check of the general path
                start = s_pos; end = j + ll;
                return 1;
            }
            // the name reaches further back than the context: general path below
        }
    }
    return 2;
}

static int swar_ref(const uint2* tab, uint32_t min_labels, uint32_t j, const uint8_t (&x)[32], uint32_t& s, uint32_t& e) {
    uint64_t b2, b1, b0;
    uint32_t w0, w1;
    memcpy(&b2, x, 8); memcpy(&b1, x + 8, 8); memcpy(&b0, x + 16, 8); memcpy(&w0, x + 24, 4); memcpy(&w1, x + 28, 4);
    return val_domain_pre(tab, min_labels, j, make_uint2(w0, w1), b0, b1, b2, s, e);
}

// ---- reference 2: the rules byte by byte. x = log[j-24, j+8): x[24..] the last label and its stop byte, x[23] down the run in front of it.
struct Labels { std::unordered_map<uint64_t, bool> alone; };   // key: the label's bytes, zero-padded
static int byte_model(const Labels& L, uint32_t min_labels, uint32_t j, const uint8_t (&x)[32], uint32_t& s, uint32_t& e) {
    uint32_t ll = 0;
    while (ll < 8 && is_dc(x[24 + ll])) ++ll;
    if (ll == 0 || ll == 8) return 2;                                        // no label here, or it does not end within the window
    for (uint32_t k = 0; k < ll; ++k) if (x[24 + k] == '.') return 0;        // a later dot owns this run
    if (!is_boundary(x[24 + ll])) return 0;
    uint64_t key = 0;
    memcpy(&key, x + 24, ll);
    const auto it = L.alone.find(key);
    if (it == L.alone.end()) return 0;                                       // no suffix ends in this label
    if (!it->second) return 2;                                               // only as part of a longer suffix
    uint32_t consumed = 0;
    while (consumed < 24 && is_dc(x[23 - consumed])) ++consumed;
    if (consumed == 24 && j != 24) return 2;                                 // the name may reach further back
    if (consumed == 0) return 0;
    const uint32_t left = 24 - consumed;
    uint32_t ndots = 0;
    bool bad = x[left] == '.' || x[left] == '-' || x[24 + ll - 1] == '-', high = false;
    for (uint32_t p = left; p < 24; ++p) {
        const unsigned c = x[p], nx = p + 1 < 24 ? x[p + 1] : 'a';           // right of x[23]: the label's first byte, taken as neither dot nor dash
        if (c == '.') { ++ndots; if (nx == '.' || nx == '-') bad = true; }   // empty label, label starting with '-'
        if (c == '-' && nx == '.') bad = true;                               // label ending with '-'
        if (c >= 0x80) high = true;
    }
    for (uint32_t k = 0; k < ll; ++k) if (x[24 + k] >= 0x80) high = true;
    if (bad || ndots == 0 || 1 + ndots < min_labels) return 0;
    if (consumed < 24 && !is_boundary(x[23 - consumed])) return 0;
    if (high) return 2;
    s = j - consumed; e = j + ll;
    return 1;
}

// ---- the table of last labels, built the way the engine builds DevDb::tld_tab
static const char* const ALONE[] = {"com", "net", "org", "io", "de", "uk", "a", "info", "museum", "xn--p1a", "co-", "c\xC3\xA9", "x1", "travel"};
static const char* const NOT_ALONE[] = {"ck", "er", "np", "sch", "kawasak", "b"};
static void add_label(std::vector<uint2>& tab, Labels& L, const char* l, bool alone) {
    uint8_t k[8] = {0};
    memcpy(k, l, strlen(l));
    uint32_t lo, hi;
    memcpy(&lo, k, 4); memcpy(&hi, k + 4, 4);
    uint32_t slot = tld_tab_slot(lo, hi);
    while ((tab[slot].y >> 24) != 0) slot = (slot + 1) & ((1u << TLD_TAB_BITS) - 1);
    tab[slot] = make_uint2(lo, hi | ((0x80u | (alone ? 1u : 0u)) << 24));
    uint64_t key;
    memcpy(&key, k, 8);
    L.alone[key] = alone;
}

// ---- inputs
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
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

static std::vector<uint2> g_tab(1u << TLD_TAB_BITS, uint2{0, 0});
static Labels g_labels;
static long g_cases = 0, g_verdict[3] = {0, 0, 0}, g_bad = 0;

static void check(const uint8_t (&x)[32], uint32_t j, uint32_t min_labels) {
    uint32_t c[8];
    memcpy(c, x, 32);
    uint32_t s0 = 0, e0 = 0, s1 = 0, e1 = 0, s2 = 0, e2 = 0;
    const int v0 = domain_rules(g_tab.data(), min_labels, j, c, s0, e0);
    const int v1 = swar_ref(g_tab.data(), min_labels, j, x, s1, e1);
    const int v2 = byte_model(g_labels, min_labels, j, x, s2, e2);
    ++g_cases;
    if (v0 >= 0 && v0 <= 2) ++g_verdict[v0];
    const bool ok = v0 == v1 && v0 == v2 && (v0 != 1 || (s0 == s1 && e0 == e1 && s0 == s2 && e0 == e2));
    if (!ok && g_bad++ < 10) {
        printf("MISMATCH planes %d [%u,%u) swar %d [%u,%u) bytes %d [%u,%u) j %u min_labels %u ctx", v0, s0, e0, v1, s1, e1, v2, s2, e2, j, min_labels);
        for (int i = 0; i < 32; ++i) printf(" %02x", x[i]);
        printf("\n");
    }
}

static void put_label(uint8_t (&x)[32], const char* label, uint8_t stop, uint32_t r) {
    const size_t n = std::min<size_t>(strlen(label), 8);
    memcpy(x + 24, label, n);
    if (n < 8) x[24 + n] = stop;
    for (size_t k = n + 1; k < 8; ++k) x[24 + k] = pick((int)((r >> (3 * k)) % NCLS), r >> k);   // behind the stop byte: anything
}

int main() {
    // ---- (a) every byte value at every position: each mask bit is the scalar class of its byte
    {
        long bad = 0;
        const uint8_t backgrounds[] = {'a', 0x00, 0xFF, '.', '-', ' '};
        for (uint8_t bg : backgrounds)
            for (int p = 0; p < 32; ++p)
                for (int v = 0; v < 256; ++v) {
                    uint8_t x[32];
                    memset(x, bg, 32);
                    x[p] = (uint8_t)v;
                    uint32_t c[8];
                    memcpy(c, x, 32);
                    const ContextMasks m = context_planes(c);
                    for (int q = 0; q < 32; ++q) {
                        const unsigned b = x[q];
                        const bool ok = ((m.DC >> q) & 1) == (unsigned)is_dc(b) && ((m.DOT >> q) & 1) == (unsigned)(b == '.') &&
                                        ((m.DASH >> q) & 1) == (unsigned)(b == '-') && ((m.HIGH >> q) & 1) == (unsigned)(b >= 0x80) &&
                                        ((m.B >> q) & 1) == (unsigned)is_boundary(b);
                        if (!ok && bad++ < 10) printf("context_planes: byte 0x%02x at %d (background 0x%02x, value 0x%02x at %d)\n", b, q, bg, v, p);
                    }
                }
        printf("context_planes: %ld wrong bits in %d x 256 x 32 records\n", bad, (int)sizeof backgrounds);
        if (bad) return 1;
    }

    for (const char* l : ALONE) add_label(g_tab, g_labels, l, true);
    for (const char* l : NOT_ALONE) add_label(g_tab, g_labels, l, false);
    const char* const probe_labels[] = {"com", "io", "a", "museum", "ck", "zz", "co-", "c\xC3\xA9"};   // suffix alone (3, 2, 1, 6 bytes), not alone, unknown, ends with '-', non-ASCII

    // ---- (b1) the 6 bytes in front of the label: every combination of the seven classes; the other look-back bytes letters
    for (uint32_t combo = 0; combo < 117649; ++combo) {   // 7^6
        uint8_t x[32];
        const uint32_t r = rnd();
        for (int i = 0; i < 18; ++i) x[i] = pick(LETTER, r >> i);
        uint32_t t = combo;
        for (int i = 0; i < 6; ++i) { x[18 + i] = pick((int)(t % NCLS), rnd()); t /= NCLS; }
        for (int li = 0; li < 3; ++li) {
            put_label(x, probe_labels[(combo + li) % 5], ' ', r);
            for (uint32_t ml = 1; ml <= 3; ++ml) { check(x, 24, ml); check(x, 1000 + combo, ml); }
        }
    }
    // the same with a boundary in front of the six bytes, so that names of 1..6 bytes in front of the label can be accepted with j > 24
    for (uint32_t combo = 0; combo < 117649; ++combo) {
        uint8_t x[32];
        const uint32_t r = rnd();
        for (int i = 0; i < 18; ++i) x[i] = pick(i >= 12 + (int)(r % 6) ? LETTER : BOUND, r >> i);
        uint32_t t = combo;
        for (int i = 0; i < 6; ++i) { x[18 + i] = pick((int)(t % NCLS), rnd()); t /= NCLS; }
        put_label(x, probe_labels[combo % 4], pick(BOUND, r), r);
        for (uint32_t ml = 1; ml <= 3; ++ml) { check(x, 24, ml); check(x, 5000 + combo, ml); }
    }
    // ---- (b2) every run length 0..24, j == 24 and j > 24, every class in front of the run, dots at every place
    for (uint32_t consumed = 0; consumed <= 24; ++consumed)
        for (int front = 0; front < NCLS; ++front)
            for (uint32_t rep = 0; rep < 400; ++rep) {
                uint8_t x[32];
                const uint32_t r = rnd();
                for (int i = 0; i < 24; ++i) x[i] = pick((int)((r >> i) % NCLS), rnd());
                for (uint32_t k = 0; k < consumed; ++k) x[23 - k] = pick(rep % 3 == 0 && k ? DIGIT : LETTER, rnd());
                if (consumed) x[23] = '.';
                if (consumed > 2 && rep % 2) x[23 - 1 - rnd() % (consumed - 1)] = pick(rep % 8 == 7 ? DASH : DOT, 0);
                if (consumed > 4 && rep % 5 == 4) x[23 - 1 - rnd() % (consumed - 1)] = pick(rep % 10 == 9 ? HIGH : DASH, rnd());
                if (consumed < 24) x[23 - consumed] = pick(front == LETTER || front == DIGIT || front == DASH || front == DOT ? BOUND : front, rnd());
                put_label(x, probe_labels[rep % 8], pick(BOUND, r), r);
                for (uint32_t ml = 1; ml <= 3; ++ml) { check(x, 24, ml); check(x, 25 + r % 100000, ml); }
            }
    // ---- (b3) every label length 1..8 with every class of stop byte
    for (uint32_t ll = 1; ll <= 8; ++ll)
        for (int stop = 0; stop < NCLS; ++stop)
            for (uint32_t rep = 0; rep < 600; ++rep) {
                uint8_t x[32];
                const uint32_t r = rnd();
                const uint32_t n = 2 + r % 20;
                for (int i = 0; i < 24; ++i) x[i] = pick(i < (int)(24 - n) ? BOUND : LETTER, rnd());
                x[23] = '.';
                if (n > 4) x[23 - 2 - rnd() % (n - 3)] = '.';
                static const char* const by_len[] = {"a", "io", "com", "info", "xn--p", "museum", "xn--p1a", "internat"};
                char label[9];
                strcpy(label, rep % 3 ? by_len[ll - 1] : "zzzzzzzz");
                label[ll] = 0;
                put_label(x, label, pick(stop, rnd()), r);
                for (uint32_t ml = 1; ml <= 3; ++ml) { check(x, 24, ml); check(x, 24 + n + r % 999, ml); }
            }
    const long constructed = g_cases;
    // ---- (b4) random contexts from a domain-heavy alphabet: 58 % letters, 8 % digits, 5 % '-', 12 % '.', 11 % boundaries, 3 % other ASCII, 3 % >= 0x80
    uint8_t alphabet[256];
    for (int i = 0; i < 256; ++i) {
        const uint32_t r = rnd(), u = (uint32_t)i * 100 / 256;
        const int cls = u < 58 ? LETTER : u < 66 ? DIGIT : u < 71 ? DASH : u < 83 ? DOT : u < 94 ? BOUND : u < 97 ? OTHER : HIGH;
        alphabet[i] = pick(cls, r >> 8);
    }
    for (long it = 0; it < 12000000; ++it) {
        uint8_t x[32];
        for (int i = 0; i < 32; i += 4) {
            const uint32_t r4 = rnd();
            for (int k = 0; k < 4; ++k) x[i + k] = alphabet[(r4 >> (8 * k)) & 0xFF];
        }
        const uint32_t r = rnd();
        if (r % 8) x[23] = '.';
        if (r % 16 >= 5) {
            const uint32_t k = (r >> 4) % 20;
            const char* l = k < 14 ? ALONE[k] : NOT_ALONE[k - 14];
            put_label(x, l, pick((r >> 9) % 4 ? BOUND : (int)((r >> 11) % NCLS), r >> 14), rnd());
        }
        check(x, (r >> 20) % 8 == 0 ? 24u : 24u + (r >> 8), 1 + (r >> 24) % 3);
    }
    printf("cases %ld (constructed %ld, random %ld)\n", g_cases, constructed, g_cases - constructed);
    printf("verdicts: 0 %ld  1 %ld  2 %ld\n", g_verdict[0], g_verdict[1], g_verdict[2]);
    printf("mismatches %ld\n", g_bad);
    if (g_bad) return 1;
    for (int v = 0; v < 3; ++v) if (g_verdict[v] < 1000) { printf("verdict %d occurs only %ld times\n", v, g_verdict[v]); return 1; }
    printf("domain_planes ok\n");
    return 0;
}
