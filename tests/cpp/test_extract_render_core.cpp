// Driver of tests/test_extract_render_host.py: runs the rules of csrc/extract_render_core.h on the host and prints what they give, for
// the Python model to compare. Built with -fsanitize=address,undefined: every candidate lies in a heap block of exactly its length and
// every record is written into a block of exactly the measured length.
//   render FILE   lines "format type hex|-"      ->  "length hex" per line (the record), after the checks below
//   keys FILE     lines "line rank start"        ->  "key line rank start" per line (pack, then unpack)
//   types                                         ->  "type rank name" for the twelve item types and one unknown
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "extract_render_core.h"

namespace X = mxy::xrender;

static int fail(const char* what, size_t line) {
    printf("FAIL line %zu: %s\n", line, what);
    return 1;
}

static int render(const char* path) {
    std::ifstream f(path);
    std::string row;
    size_t no = 0;
    while (std::getline(f, row)) {
        ++no;
        std::istringstream in(row);
        uint32_t format, type;
        std::string hex;
        in >> format >> type >> hex;
        const size_t n = hex == "-" ? 0 : hex.size() / 2;
        uint8_t* text = (uint8_t*)malloc(n ? n : 1);   // exactly the candidate: a read past it is reported
        for (size_t i = 0; i < n; ++i) text[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        const uint64_t esc = X::count_escapes(format, text, (uint32_t)n);
        const uint64_t want = X::record_len(format, type, (uint32_t)n, esc);
        // the parts add up to the record
        uint8_t head[X::HEAD_MAX], tail[X::TAIL_MAX];
        if (X::head_put(format, type, head) != X::head_len(format, type)) return fail("head_put != head_len", no);
        if (X::tail_put(format, tail) != X::tail_len(format)) return fail("tail_put != tail_len", no);
        if (X::head_len(format, type) > X::HEAD_MAX || X::tail_len(format) > X::TAIL_MAX) return fail("part longer than its bound", no);
        // a block of exactly the length
        uint8_t* block = (uint8_t*)malloc(want);
        memset(block, 0xEE, want);
        if (X::record_put(format, type, text, (uint32_t)n, block, 0, want) != want) return fail("record_put != record_len", no);
        // a block that ends one byte early, behind an offset: the length is the same, the bytes in front are the same, nothing at `end`
        const uint64_t off = 5;
        std::vector<uint8_t> shortb(off + want, 0xEE);
        if (X::record_put(format, type, text, (uint32_t)n, shortb.data(), off, off + want - 1) != want) return fail("length depends on the capacity", no);
        if (memcmp(shortb.data() + off, block, want - 1) != 0 || shortb[off + want - 1] != 0xEE) return fail("a byte at or behind the end", no);
        for (uint64_t k = 0; k < off; ++k) if (shortb[k] != 0xEE) return fail("a byte in front of the record", no);
        printf("%" PRIu64 " ", want);
        for (uint64_t k = 0; k < want; ++k) printf("%02x", block[k]);
        printf("\n");
        free(block);
        free(text);
    }
    printf("extract_render_core ok\n");
    return 0;
}

static int keys(const char* path) {
    std::ifstream f(path);
    uint64_t line, rank, start;
    while (f >> line >> rank >> start) {
        const unsigned long long k = X::key_pack((uint32_t)line, (uint32_t)rank, (uint32_t)start);
        printf("%llu %u %u %u\n", k, X::key_line(k), X::key_rank(k), X::key_start(k));
    }
    printf("extract_render_core ok\n");
    return 0;
}

static int types() {
    for (uint32_t t = 0; t <= 12; ++t) {
        uint8_t name[X::TYPE_NAME_MAX + 1] = {0};
        const uint32_t n = X::name_put(t, name);
        if (n > X::TYPE_NAME_MAX || n != X::name_len(t)) return fail("name length", t);
        printf("%u %u %s\n", t, X::rank(t), (const char*)name);
    }
    printf("bits %u %u %u max_len %u\n", X::LINE_BITS, X::RANK_BITS, X::START_BITS, X::MAX_LEN);
    printf("extract_render_core ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "render" && argc > 2) return render(argv[2]);
    if (what == "keys" && argc > 2) return keys(argv[2]);
    if (what == "types") return types();
    fprintf(stderr, "usage: test_extract_render_core render FILE | keys FILE | types\n");
    return 2;
}
