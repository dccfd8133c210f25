// CPU check of the parts of k_anchor's front end that decide where the boundary plane and the long-token chain are needed
// (matchy_amd/csrc/anchor_planes.h): boundary_plane(), the "neither digit nor '.'" plane, the IPv4 anchor plane against the
// formula it replaced, the long-token trigger and the exact chain. Arguments: log files (name=path) to run the IPv4 plane
// and the trigger over; "nginx=..." also carries the bound on how often the trigger may fire.
// Build: g++ -O1 -std=c++17 -I matchy_amd/csrc tests/cpp/test_anchor_trigger.cpp -o /tmp/test_anchor_trigger
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "anchor_planes.h"

using namespace mxy;

static int bad = 0;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

// ---- a block the way the wave sees it: planes of the 64 lanes, previous / next dword words with the row wrap
struct BlockPlanes { ClassPlanes cl[64]; uint32_t N[64]; };
static void block_planes(const uint8_t* blk, BlockPlanes& bp) {
    for (int L = 0; L < 64; ++L) {
        uint32_t w[8];
        for (int q = 0; q < 8; ++q) memcpy(&w[q], blk + 256 * q + 4 * L, 4);
        bit_transpose8(w);
        bp.cl[L] = classify_planes(w, false);
        bp.N[L] = nondigit_nondot_plane(bp.cl[L].D, bp.cl[L].T);
    }
}
// plane_prev_dword / plane_next_dword of k_anchor.hip
template <class Get> static void prev_words(Get get, uint32_t& carry, uint32_t (&pv)[64]) {
    const uint32_t s63 = get(63);
    pv[0] = ((s63 << 1) & 0xFEFEFEFEu) | ((carry >> 7) & 0x01010101u);
    for (int L = 1; L < 64; ++L) pv[L] = get(L - 1);
    carry = s63;
}
// `first_of_next`: the word of lane 0 of the block behind this one (its row 0 follows row 7 of lane 63); nullptr = not staged yet, the
// wave takes "anything" there
template <class Get> static void next_words(Get get, const uint32_t* first_of_next, uint32_t (&nv)[64]) {
    for (int L = 0; L < 63; ++L) nv[L] = get(L + 1);
    nv[63] = ((get(0) >> 1) & 0x7F7F7F7Fu) | (first_of_next ? (*first_of_next << 7) & 0x80808080u : 0x80808080u);
}

struct V4Stats { unsigned long long old_n = 0, new_n = 0, missing = 0, extra_inside = 0; };
// The whole buffer as one segment (n a multiple of 2048). `staged_ahead`: the pattern itself, with the true bytes behind the end of a
// block; without it the look-ahead past the block is "anything", as in the wave (the drain sees those anchors again when the next
// block is there), for the old formula and the new one alike.
static V4Stats ipv4_planes(const uint8_t* buf, size_t n, bool staged_ahead) {
    V4Stats st;
    uint32_t cB = 0x80808080u, cN = 0x80808080u, cD = 0;   // in front of the buffer: a boundary
    static BlockPlanes two[2];
    if (n >= AB_BLOCK) block_planes(buf, two[0]);
    for (size_t b = 0, i = 0; b + AB_BLOCK <= n; b += AB_BLOCK, ++i) {
        const BlockPlanes& bp = two[i & 1];
        const bool have_next = b + 2 * AB_BLOCK <= n;
        if (have_next) block_planes(buf + b + AB_BLOCK, two[(i + 1) & 1]);
        const BlockPlanes& nx = two[(i + 1) & 1];
        const bool ahead = staged_ahead && have_next;
        uint32_t pvB[64], pvN[64], pvD[64], nvD[64], nvT[64];
        prev_words([&](int L) { return bp.cl[L].B; }, cB, pvB);
        prev_words([&](int L) { return bp.N[L]; }, cN, pvN);
        prev_words([&](int L) { return bp.cl[L].D; }, cD, pvD);
        next_words([&](int L) { return bp.cl[L].D; }, ahead ? &nx.cl[0].D : nullptr, nvD);
        next_words([&](int L) { return bp.cl[L].T; }, ahead ? &nx.cl[0].T : nullptr, nvT);
        for (int L = 0; L < 64; ++L) {
            const ClassPlanes& c = bp.cl[L];
            const uint32_t Dm1 = plane_back<1>(c.D, pvD[L]);
            // the formula this replaces: boundary 2..4 back, digit at j+1
            const uint32_t old_back = Dm1 & (plane_back<2>(c.B, pvB[L]) | plane_back<3>(c.B, pvB[L]) | plane_back<4>(c.B, pvB[L]));
            const uint32_t old_ahead = plane_ahead<1>(c.D, nvD[L]) & (plane_ahead<2>(c.T, nvT[L]) | plane_ahead<3>(c.T, nvT[L]) | plane_ahead<4>(c.T, nvT[L]));
            const uint32_t f_old = c.T & old_back & old_ahead;
            const uint32_t f_new = ipv4_anchor_plane(c.T, Dm1, bp.N[L], pvN[L], nvT[L]);
            st.old_n += __builtin_popcount(f_old);
            st.new_n += __builtin_popcount(f_new);
            st.missing += __builtin_popcount(f_old & ~f_new);
            // anchors the new plane adds in front of the last four bytes of the block (where the look-ahead is complete either way)
            for (uint32_t e = f_new & ~f_old; e; e &= e - 1) st.extra_inside += plane_bit_offset(L, __builtin_ctz(e)) + 4 < AB_BLOCK;
        }
    }
    return st;
}

// ---- long tokens
static bool is_alnum(unsigned b) { return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'); }
// per-dword reference of the exact chain: stream[64 + 64 q + L] = dword L of row q, stream[L] = row 7 of the previous block
static void chain_reference(const uint32_t (&a4)[64], const uint32_t (&aprev)[64], uint32_t (&rows)[64]) {
    bool stream[64 + 512];
    for (int L = 0; L < 64; ++L) stream[L] = aprev[L] & 1;
    for (int q = 0; q < 8; ++q) for (int L = 0; L < 64; ++L) stream[64 + 64 * q + L] = (a4[L] >> q) & 1;
    for (int L = 0; L < 64; ++L) {
        rows[L] = 0;
        for (int q = 0; q < 8; ++q) {
            const int s = 64 + 64 * q + L;
            bool all = true;
            for (int k = 1; k <= 5; ++k) all = all && stream[s - k];
            rows[L] |= (uint32_t)all << q;
        }
    }
}
struct TokStats { unsigned long long blocks = 0, fired = 0, chain = 0; };
static void check_token_block(const uint32_t (&a4)[64], const uint32_t (&aprev)[64], TokStats& st, const char* what) {
    uint32_t r[64], want[64];
    tok_chain5(a4, aprev, r);
    chain_reference(a4, aprev, want);
    bool any = false;
    for (int L = 0; L < 64; ++L) {
        if (tok_chain_rows(r[L]) != want[L]) FAIL("%s: exact chain differs from the per-dword loop, block %llu lane %d: %02x want %02x", what, st.blocks, L, tok_chain_rows(r[L]), want[L]);
        any = any || want[L] != 0;
    }
    const bool trig = tok_trigger(a4, aprev);
    if (any && !trig) FAIL("%s: block %llu has five all-alphanumeric dwords in a row and the trigger does not fire", what, st.blocks);
    st.blocks += 1; st.fired += trig; st.chain += any;
}
static TokStats token_file(const uint8_t* buf, size_t n, const char* what) {
    TokStats st;
    uint32_t aprev[64] = {0};
    for (size_t b = 0; b + AB_BLOCK <= n; b += AB_BLOCK) {
        uint32_t a4[64];
        for (int L = 0; L < 64; ++L) {
            uint32_t w[8];
            for (int q = 0; q < 8; ++q) memcpy(&w[q], buf + b + 256 * q + 4 * L, 4);
            uint32_t direct = 0;
            for (int q = 0; q < 8; ++q) {
                const uint8_t* d = buf + b + 256 * q + 4 * L;
                direct |= (uint32_t)(is_alnum(d[0]) && is_alnum(d[1]) && is_alnum(d[2]) && is_alnum(d[3])) << q;
            }
            bit_transpose8(w);
            a4[L] = tok_a4(classify_planes(w, false).LD, w[7]);
            if (a4[L] != direct) FAIL("%s: tok_a4 differs from the byte-wise test at %zu lane %d", what, b, L);
        }
        check_token_block(a4, aprev, st, what);
        for (int L = 0; L < 64; ++L) aprev[L] = a4[L] >> 7;
    }
    return st;
}

int main(int argc, char** argv) {
    // 1. boundary_plane == classify_planes().B, and "neither digit nor '.'" contains it: all 256 byte values in every byte lane and row
    for (int v = 0; v < 256; ++v)
        for (int slot = 0; slot < 32; ++slot) {
            uint8_t bytes[32];
            for (int i = 0; i < 32; ++i) bytes[i] = (uint8_t)((v * 7 + i * 13 + 1) & 0xFF);   // neighbours: something else
            bytes[slot] = (uint8_t)v;
            uint32_t w[8];
            for (int q = 0; q < 8; ++q) memcpy(&w[q], bytes + 4 * q, 4);
            bit_transpose8(w);
            for (int wide = 0; wide < 2; ++wide) {
                const ClassPlanes c = classify_planes(w, wide != 0);
                const uint32_t B = boundary_plane(w), N = nondigit_nondot_plane(c.D, c.T);
                if (B != c.B) FAIL("boundary_plane differs from classify_planes().B for byte 0x%02x in slot %d", v, slot);
                if (c.B & ~N) FAIL("a boundary byte outside the neither-digit-nor-dot plane: 0x%02x in slot %d", v, slot);
                for (int i = 0; i < 32; ++i) {
                    const unsigned x = bytes[i], t = 8 * (i & 3) + (i >> 2);
                    if (((N >> t) & 1) != (unsigned)!((x >= '0' && x <= '9') || x == '.')) FAIL("neither-digit-nor-dot plane wrong for byte 0x%02x", x);
                }
            }
        }
    // 2. IPv4 anchor plane: a superset of the old one at every position of random bytes (all byte values; digits, dots and separators only)
    std::mt19937 rng(2024);
    {
        std::vector<uint8_t> buf(64 * AB_BLOCK);
        for (int mode = 0; mode < 2; ++mode) {
            static const char dense[] = "0123456789....  /:ax";
            for (auto& c : buf) c = mode ? (uint8_t)dense[rng() % (sizeof(dense) - 1)] : (uint8_t)(rng() & 0xFF);
            for (int staged = 0; staged < 2; ++staged) {
                const V4Stats st = ipv4_planes(buf.data(), buf.size(), staged != 0);
                if (st.missing) FAIL("random bytes (mode %d): %llu old IPv4 anchors are not in the new plane", mode, st.missing);
                if (mode && st.old_n == 0) FAIL("random digits and dots produced no anchor at all");
                printf("ipv4 random mode %d staged %d: old %llu new %llu\n", mode, staged, st.old_n, st.new_n);
            }
        }
    }
    // 3. token trigger and exact chain on random a4 blocks
    {
        // one million blocks, a third at each density; a bit is set when a byte of the generator's output lies under the threshold
        // ... and 100 000 more at 0.15, where most blocks have no five in a row (at 0.7 and 0.95 every block has)
        const double dens[4] = {0.3, 0.7, 0.95, 0.15};
        std::mt19937_64 r64(77);
        for (int di = 0; di < 4; ++di) {
            TokStats st;
            const unsigned thr = (unsigned)(dens[di] * 256.0);
            auto bits8 = [&]() { uint64_t v = r64(); uint32_t o = 0; for (int q = 0; q < 8; ++q) o |= (uint32_t)(((v >> (8 * q)) & 0xFF) < thr) << q; return o; };
            const int per = di == 3 ? 100000 : 1000000 / 3 + (di == 0);
            for (int n = 0; n < per; ++n) {
                uint32_t a4[64], aprev[64];
                for (int L = 0; L < 64; ++L) a4[L] = bits8();
                for (int L = 0; L < 64; L += 8) { const uint32_t v = bits8(); for (int k = 0; k < 8; ++k) aprev[L + k] = (v >> k) & 1; }
                check_token_block(a4, aprev, st, "random");
            }
            printf("token random density %.2f: %llu blocks, trigger %llu, chain %llu\n", dens[di], st.blocks, st.fired, st.chain);
        }
    }
    // 4. the log files
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq || !strncmp(argv[i], "blocks=", 7)) continue;
        const std::string name(argv[i], eq - argv[i]);
        FILE* f = fopen(eq + 1, "rb");
        if (!f) { FAIL("cannot open %s", eq + 1); continue; }
        std::vector<uint8_t> buf;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        buf.resize((buf.size() + AB_BLOCK - 1) / AB_BLOCK * AB_BLOCK, (uint8_t)' ');   // positions past the end read as ' '
        // the pattern over the log: not one anchor more than the old formula lists
        const V4Stats v4 = ipv4_planes(buf.data(), buf.size(), true);
        if (v4.missing) FAIL("%s: %llu old IPv4 anchors are not in the new plane", name.c_str(), v4.missing);
        if (v4.new_n > v4.old_n) FAIL("%s: IPv4 anchors rose from %llu to %llu", name.c_str(), v4.old_n, v4.new_n);
        // the wave's view (nothing known behind the block): a superset again, and what it adds stands in the last four bytes of a block,
        // where any "digit '.'" with a letter in front passes until the next block is staged
        const V4Stats wv = ipv4_planes(buf.data(), buf.size(), false);
        if (wv.missing) FAIL("%s: %llu old IPv4 anchors are not in the new plane (look-ahead ends with the block)", name.c_str(), wv.missing);
        if (wv.extra_inside) FAIL("%s: %llu new IPv4 anchors in front of the last four bytes of a block", name.c_str(), wv.extra_inside);
        printf("%s: look-ahead ending with the block: ipv4 anchors old %llu new %llu\n", name.c_str(), wv.old_n, wv.new_n);
        const TokStats tk = token_file(buf.data(), buf.size(), name.c_str());
        const double pct = tk.blocks ? 100.0 * (double)tk.fired / (double)tk.blocks : 0.0;
        printf("%s: ipv4 anchors old %llu new %llu; token trigger fires in %llu of %llu blocks = %.2f %% (exact chain nonzero in %llu)\n",
               name.c_str(), v4.old_n, v4.new_n, tk.fired, tk.blocks, pct, tk.chain);
        if (name == "nginx" && !(pct < 25.0)) FAIL("nginx: the token trigger fires in %.2f %% of the blocks, the bound is 25 %%", pct);
    }
    if (bad) { printf("FAILED: %d mismatches\n", bad); return 1; }
    printf("anchor_trigger ok\n");
    return 0;
}
