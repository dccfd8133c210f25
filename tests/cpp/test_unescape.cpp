// CPU check of matchy_amd/csrc/unescape_core.h.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I matchy_amd/csrc tests/cpp/test_unescape.cpp -o /tmp/test_unescape
//   test_unescape cases IN OUT   decodes every case of IN (tests/unescape_cases.py write_case_file) tile by tile, the way the kernels
//                                partition the work: JSON first gets the code of every full tile (tile_state_code) and the states
//                                from them, in order and again through fn_compose, and both are held against esc walked byte by byte
//                                over the whole input; then tile_count of every tile, an exclusive prefix, and tile_write of every
//                                tile into its own range of a buffer of exactly the total (a pass that disagrees with the other
//                                stops the sanitized program or fails the check). Modes 3 is two such runs. OUT: per case u32
//                                length, u32 escapes, u32 U+FFFD written, u32 LF escapes, the bytes.
#include <cstdio>
#include <cstring>
#include <vector>

#include "unescape_core.h"

using namespace mxy;
using namespace mxy::unescape;

static int bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the states of all tiles from the codes of the full ones, held against the definition
static std::vector<uint32_t> states_of(const std::vector<uint8_t>& data, uint32_t c) {
    const size_t len = data.size();
    const uint64_t n_tiles = tiles(len);
    std::vector<uint32_t> state(n_tiles, 0), codes;
    for (uint64_t t = 0; t + 1 < n_tiles; ++t) {
        codes.push_back(tile_state_code(data.data(), len, t));
        state[t + 1] = code_apply(codes[t], state[t]);
    }
    // esc of every byte, walked from the first one: esc[i] = data[i - 1] == '\\' && !esc[i - 1]
    std::vector<uint8_t> esc(len + 1, 0);
    for (size_t i = 1; i <= len; ++i) esc[i] = data[i - 1] == '\\' && !esc[i - 1];
    uint32_t f = FN_IDENTITY;   // the composition of the codes in front of tile t, as the scan kernels build it
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const size_t ts = t * TILE_BYTES;
        uint32_t want = esc[ts];
        for (uint32_t k = 0; k < 6; ++k) want |= (ts >= 6 ? (uint32_t)esc[ts - 6 + k] : 0u) << (1 + k);
        CHECK(state[t] == want, "case %u tile %llu: state %#x, walked %#x", c, (unsigned long long)t, state[t], want);
        CHECK((f & 1u) == esc[ts], "case %u tile %llu: composed function %u, esc %u", c, (unsigned long long)t, f, esc[ts]);
        if (t + 1 < n_tiles) f = fn_compose(f, fn_of(codes[t]));
    }
    return state;
}

// one run of the pass
static bool run_pass(const std::vector<uint8_t>& data, uint32_t mode, uint32_t c, std::vector<uint8_t>& text, Counters& ctr) {
    const size_t len = data.size();   // exactly len bytes: a read behind the input stops the program
    const uint64_t n_tiles = tiles(len);
    std::vector<uint32_t> state(n_tiles, 0);
    if (mode == MODE_JSON) state = states_of(data, c);
    std::vector<uint32_t> prefix(n_tiles + 1, 0);
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const uint32_t k = tile_count(data.data(), len, mode, t, state[t], &ctr);
        CHECK(k <= TILE_OUT_MAX, "case %u tile %llu: %u bytes", c, (unsigned long long)t, k);
        prefix[t + 1] = prefix[t] + k;
    }
    const uint32_t total = prefix[n_tiles];
    CHECK(total <= len, "case %u: %u bytes from %zu", c, total, len);
    text.assign(total, 0);
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint8_t tile[TILE_OUT_MAX];
        const uint32_t k = tile_write(data.data(), len, mode, t, state[t], tile);
        CHECK(k == prefix[t + 1] - prefix[t], "case %u tile %llu: the write pass gives %u bytes, the count pass %u", c, (unsigned long long)t, k, prefix[t + 1] - prefix[t]);
        if (k != prefix[t + 1] - prefix[t]) return false;
        if (k) memcpy(text.data() + prefix[t], tile, k);
    }
    return true;
}

static int run_cases(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    FILE* o = fopen(out_path, "wb");
    if (!f || !o) { printf("cannot open files\n"); return 2; }
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 2;
        const uint32_t modes = head[0], len = head[1];
        std::vector<uint8_t> data(len), text;
        if (len && fread(data.data(), 1, len, f) != len) return 2;
        Counters ctr;
        for (const uint32_t mode : {MODE_JSON, MODE_PERCENT}) {
            if (!(modes & mode)) continue;
            if (!run_pass(data, mode, c, text, ctr)) return 1;
            data = text;
        }
        const uint32_t out[4] = {(uint32_t)text.size(), (uint32_t)ctr.escapes, (uint32_t)ctr.replaced, (uint32_t)ctr.lf_escapes};
        fwrite(out, 4, 4, o);
        if (!text.empty()) fwrite(text.data(), 1, text.size(), o);
    }
    fclose(f); fclose(o);
    if (!bad) printf("unescape cases ok: %u\n", n_cases);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "cases")) return run_cases(argv[2], argv[3]);
    printf("usage: test_unescape cases IN OUT\n");
    return 2;
}
