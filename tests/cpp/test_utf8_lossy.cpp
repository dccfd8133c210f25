// utf8_lossy.h (the "input_line" conversion of the NDJSON renderer) alone: every line of stdin is one case in hex; the converted bytes
// go to stdout in hex, one line per case. The cases are copied into heap blocks of exactly their size, so that a read past the end of
// the input is caught by AddressSanitizer.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include "utf8_lossy.h"

int main() {
    std::string line;
    size_t cases = 0;
    while (std::getline(std::cin, line)) {
        const size_t n = line.size() / 2;
        std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
        for (size_t i = 0; i < n; ++i) in[i] = (uint8_t)std::stoul(line.substr(2 * i, 2), nullptr, 16);
        std::string out;
        mxy::utf8_lossy_append(in.get(), n, out);
        for (unsigned char c : out) printf("%02x", c);
        printf("\n");
        ++cases;
    }
    fprintf(stderr, "utf8_lossy: %zu cases\n", cases);
    return 0;
}
