// Drives csrc/gz_packer.h alone (no library, no GPU): `test_gz_packer BATCH_BYTES MEMBERS MAX_MEMBER MAX_CARRY PATH...` prints the derived
// bounds — "bounds <batch_bytes> <max_member> <carry_cap> <max_text>" — and then the calls of the packer in order, one per line:
// "pack <input>:<offset>:<len>:<isize>:<members> ..." and "single <input>". MEMBERS is 0 or 1 (--gz-members); MAX_MEMBER and MAX_CARRY are
// the two overrides, "-" = absent. tests/test_gz_packer_host.py builds it with -fsanitize=address,undefined and compares the lines with
// the Python model of tests/gz_packer_cases.py.
// A PATH with a leading '!': the file loses its last byte between the packer's stat and its read.
// Every pack is checked here against the files themselves: its files lie end to end from offset 0 and their bytes are the files'.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../matchy_amd/csrc/gz_packer.h"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    auto override_of = [](const char* s) { return strcmp(s, "-") == 0 ? std::optional<uint64_t>() : std::optional<uint64_t>(strtoull(s, nullptr, 10)); };
    mxy::GzPacker packer;
    packer.bounds = mxy::gz_bounds(strtoull(argv[1], nullptr, 10), override_of(argv[3]), override_of(argv[4]));
    packer.members = atoi(argv[2]) != 0;
    const mxy::GzBounds& b = packer.bounds;
    printf("bounds %zu %zu %zu %llu\n", b.batch_bytes, b.max_member, b.carry_cap, (unsigned long long)b.max_text);
    std::vector<std::string> paths;
    std::vector<char> shrinks;
    for (int i = 5; i < argc; ++i) { shrinks.push_back(argv[i][0] == '!'); paths.push_back(argv[i] + (argv[i][0] == '!' ? 1 : 0)); }
    packer.read_file = [&](const std::string& path, uint8_t* dst, size_t size) {
        for (size_t i = 0; i < paths.size(); ++i)
            if (shrinks[i] && paths[i] == path && truncate(path.c_str(), (off_t)size - 1) != 0) { printf("cannot shrink %s\n", path.c_str()); exit(1); }
        return mxy::pack_read_file(path, dst, size);
    };
    packer.on_pack = [&](const std::vector<uint8_t>& packed, const std::vector<mxy::GzFile>& files) {
        printf("pack");
        uint64_t at = 0;
        for (const mxy::GzFile& g : files) {
            printf(" %zu:%llu:%u:%u:%u", g.input, (unsigned long long)g.offset, g.len, g.isize, g.members);
            std::vector<uint8_t> file(g.len);
            const bool same = g.offset == at && at + g.len <= packed.size() && mxy::pack_read_file(paths[g.input], file.data(), g.len) == (long long)g.len &&
                              memcmp(file.data(), packed.data() + at, g.len) == 0;
            if (!same) { printf("\nfile %zu of the pack does not lie at %llu with its own bytes\n", g.input, (unsigned long long)at); exit(1); }
            at += g.len;
        }
        printf("\n");
        if (at != packed.size()) { printf("the pack has %zu bytes, its files %llu\n", packed.size(), (unsigned long long)at); exit(1); }
    };
    packer.not_eligible = [](size_t i) { printf("single %zu\n", i); };
    for (size_t i = 0; i < paths.size(); ++i) packer.take(i, paths[i]);
    packer.flush();
    return 0;
}
