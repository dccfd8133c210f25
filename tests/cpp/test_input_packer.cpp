// Drives csrc/input_packer.h alone (no library, no GPU): `test_input_packer BATCH_BYTES PATH...` prints the calls of pack_inputs in
// order, one per line — "pack <hex of the bytes> <input>:<start>:<appended> ...", "single <input>", "error <input>" — and the totals.
// tests/test_segments_host.py builds it with -fsanitize=address,undefined and compares the lines with the Python model.
// BATCH_BYTES with a leading '!': the process allows itself one more file descriptor only, and the first pack that goes out takes it
// and keeps it — every file behind that pack can be stat'ed and cannot be opened, whoever runs the test.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <sys/resource.h>

#include "../../matchy_amd/csrc/input_packer.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const bool starve = argv[1][0] == '!';
    struct rlimit before;
    int taken = -1;
    const size_t batch_bytes = strtoull(argv[1] + (starve ? 1 : 0), nullptr, 10);
    if (starve) {
        const int probe = open("/dev/null", O_RDONLY);   // the lowest free descriptor
        if (probe < 0) return 3;
        close(probe);
        if (getrlimit(RLIMIT_NOFILE, &before) != 0) return 3;
        struct rlimit rl = before;
        rl.rlim_cur = (rlim_t)probe + 1;
        if (setrlimit(RLIMIT_NOFILE, &rl) != 0) return 3;
    }
    std::vector<std::string> paths(argv + 2, argv + argc);
    const mxy::PackStats st = mxy::pack_inputs(
        paths, batch_bytes,
        [&](mxy::InputPack&& p) {
            printf("pack ");
            for (size_t i = 0; i < p.len; ++i) printf("%02x", p.data[i]);
            size_t appended = 0;
            for (const mxy::PackedInput& pi : p.inputs) { printf(" %zu:%u:%d", pi.input, pi.start, pi.appended ? 1 : 0); appended += pi.appended; }
            printf("\n");
            if (appended != p.appended) { printf("appended %zu != %zu\n", appended, p.appended); exit(1); }
            for (size_t i = 0; i < 16; ++i) p.data[p.len + i] = 0;   // the spare bytes behind the batch are the pack's
            if (starve && taken < 0 && (taken = open("/dev/null", O_RDONLY)) < 0) { printf("no descriptor left to take\n"); exit(1); }
        },
        [&](size_t i) { printf("single %zu\n", i); },
        [&](size_t i, int) { printf("error %zu\n", i); });
    printf("stats %zu %zu\n", st.inputs, st.packs);
    if (starve) {   // the leak check at exit opens files
        if (taken >= 0) close(taken);
        (void)setrlimit(RLIMIT_NOFILE, &before);
    }
    return 0;
}
