// Stand-alone check of csrc/whole_lines_core.h on the host: reads a buffer from the file named on the command line and prints what the
// rules make of it, for tests/test_whole_lines_host.py to hold against the Python model. The verdicts are produced the way the kernels
// produce them: the line ends from the positions of the '\n' bytes, UTF-8 validity per byte with the verdict attributed to the line the
// byte lies in, classification over the query without its '\r'.
//   L <line> <start> <query end> <class: 0 string, 1 IPv4, 2 IPv6> <1: not valid UTF-8> <address bytes in hex, or ->
//   N <lines> <newlines>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../matchy_amd/csrc/whole_lines_core.h"

using namespace mxy;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: test_whole_lines_core FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> buf;
    uint8_t tmp[4096];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    // an exact-size copy: a read past the end is a heap overflow the sanitizer sees
    std::vector<uint8_t> data(buf.begin(), buf.end());
    data.shrink_to_fit();
    const uint32_t len = (uint32_t)data.size();
    std::vector<uint32_t> ends;
    for (uint32_t i = 0; i < len; ++i) if (data[i] == '\n') ends.push_back(i);
    const uint32_t newlines = (uint32_t)ends.size();
    const uint32_t lines = wl::line_count(len, newlines, len ? data[len - 1] : 0);
    std::vector<uint8_t> invalid(lines, 0);
    {
        uint32_t line = 0;   // '\n' bytes in front of byte i
        for (uint32_t i = 0; i < len; ++i) {
            if (wl::utf8_byte_bad_at(data.data(), len, i)) invalid[line] = 1;
            if (data[i] == '\n') ++line;
        }
    }
    for (uint32_t r = 0; r < lines; ++r) {
        const uint32_t s = wl::line_start(ends.data(), r);
        const uint32_t e = wl::query_end(data.data(), s, wl::line_end(ends.data(), newlines, len, r));
        // the query alone, exact size again: classification must not read outside it
        std::vector<uint8_t> q(data.begin() + s, data.begin() + e);
        q.shrink_to_fit();
        IpAddr a;
        const wl::QueryClass c = wl::classify(q.data(), (uint32_t)q.size(), a);
        printf("L %u %u %u %u %u ", r, s, e, (unsigned)c, (unsigned)invalid[r]);
        if (c == wl::Q_STRING) printf("-");
        else for (int k = 0; k < (a.v6 ? 16 : 4); ++k) printf("%02x", a.b[k]);
        printf("\n");
    }
    printf("N %u %u\n", lines, newlines);
    return 0;
}
