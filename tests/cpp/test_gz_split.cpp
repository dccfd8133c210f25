// CPU: the member split and the file plan of a gz scan of multi-member files (matchy_amd/csrc/gz_plan.h: gz_split_members,
// gz_plan_files) printed for tests/test_gz_files_host.py to hold against its model. Built with -fsanitize=address,undefined; every
// input lies in a heap block of exactly its length, so a read behind a file's end stops the program.
//
//   test_gz_split split CASES    CASES: u32 n, then per case u32 len, u32 (unused), bytes — one FILE per case
//                                prints "file i c0 c1 ..." per file: the offsets where its members start
//   test_gz_split plan CASES     the cases are the files of ONE pack, end to end
//                                prints "member i file body body_len start cap status", "file f first start cap", "order ...", "total N";
//                                exit 1 and the message for a refused plan
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gz_plan.h"

using namespace mxy;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_gz_split split|plan CASES\n"); return 2; }
    const bool plan_mode = !strcmp(argv[1], "plan");
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror("open"); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<std::vector<uint8_t>> cases(n);
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        cases[c].resize(hdr[0]);
        if (hdr[0] && fread(cases[c].data(), 1, hdr[0], f) != hdr[0]) return 2;
    }
    fclose(f);
    int rc = 0;
    if (!plan_mode) {
        std::vector<uint64_t> cuts;
        for (uint32_t c = 0; c < n; ++c) {
            const size_t len = cases[c].size();
            uint8_t* p = (uint8_t*)malloc(len ? len : 1);
            if (len) memcpy(p, cases[c].data(), len);
            gz_split_members(p, len, cuts);
            printf("file %u", c);
            for (uint64_t q : cuts) printf(" %llu", (unsigned long long)q);
            printf("\n");
            if (cuts.empty() || cuts[0] != 0 || cuts.size() > len / 18 + 1) { printf("file %u: bad cut list\n", c); rc = 3; }
            free(p);
        }
        return rc;
    }
    std::vector<GzFileIn> files;
    size_t total = 0;
    for (const auto& c : cases) { files.push_back(GzFileIn{total, c.size()}); total += c.size(); }
    uint8_t* packed = (uint8_t*)malloc(total ? total : 1);
    for (size_t c = 0; c < cases.size(); ++c) if (!cases[c].empty()) memcpy(packed + files[c].offset, cases[c].data(), cases[c].size());
    GzFilesPlan plan;
    std::string err;
    if (!gz_plan_files(packed, total, files.data(), files.size(), plan, err)) { printf("refused: %s\n", err.c_str()); rc = 1; }
    else {
        for (size_t i = 0; i < plan.members.size(); ++i) {
            const GzPlanned& g = plan.members[i];
            printf("member %zu %u %llu %u %u %u %d\n", i, plan.member_file[i], (unsigned long long)g.body, g.body_len, g.start, g.cap, g.status);
        }
        for (size_t k = 0; k < files.size(); ++k) printf("file %zu %u %u %u\n", k, plan.first_member[k], plan.starts[k], plan.caps[k]);
        if (plan.first_member.size() != files.size() + 1 || plan.first_member.back() != plan.members.size()) { printf("first_member does not close\n"); rc = 3; }
        printf("order");
        for (uint32_t i : plan.order) printf(" %u", i);
        printf("\ntotal %llu\n", (unsigned long long)plan.total);
    }
    // a file outside the buffer, by offset and by length, an offset that would wrap a 64-bit sum, a file of 4 GiB, and an empty table
    const GzFileIn outside[4] = {{total + 1, 0}, {0, total + 1}, {~0ull - 3, 8}, {0, 1ull << 32}};
    for (const GzFileIn& m : outside) if (gz_plan_files(packed, total, &m, 1, plan, err)) { printf("a file outside the buffer was planned\n"); rc = 3; }
    if (gz_plan_files(packed, total, files.data(), 0, plan, err)) { printf("an empty table was planned\n"); rc = 3; }
    if (gz_plan_files(packed, total, nullptr, 1, plan, err)) { printf("a null table was planned\n"); rc = 3; }
    free(packed);
    return rc;
}
