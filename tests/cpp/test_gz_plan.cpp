// CPU: the host plan of a gz scan (matchy_amd/csrc/gz_plan.h) printed for a pack, for tests/test_inflate_core_host.py to hold against
// its model. Built with -fsanitize=address,undefined; the pack lies in a heap block of exactly its length.
//
//   test_gz_plan CASES     CASES: u32 n, then per case u32 len, u32 out_len, bytes — the members of ONE pack, end to end
//   prints "member i body body_len start cap status" per member, "order ...", "total N"; exit 1 and the message for a refused plan
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gz_plan.h"

using namespace mxy;

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: test_gz_plan CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<GzMemberIn> members;
    std::vector<uint8_t> bytes;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        members.push_back(GzMemberIn{bytes.size(), hdr[0], hdr[1]});
        bytes.resize(bytes.size() + hdr[0]);
        if (hdr[0] && fread(bytes.data() + bytes.size() - hdr[0], 1, hdr[0], f) != hdr[0]) return 2;
    }
    fclose(f);
    uint8_t* packed = (uint8_t*)malloc(bytes.empty() ? 1 : bytes.size());
    for (size_t i = 0; i < bytes.size(); ++i) packed[i] = bytes[i];
    GzPlan plan;
    std::string err;
    int rc = 0;
    if (!gz_plan(packed, bytes.size(), members.data(), members.size(), plan, err)) { printf("refused: %s\n", err.c_str()); rc = 1; }
    else {
        for (size_t i = 0; i < plan.members.size(); ++i) {
            const GzPlanned& g = plan.members[i];
            printf("member %zu %llu %u %u %u %d\n", i, (unsigned long long)g.body, g.body_len, g.start, g.cap, g.status);
            if (plan.starts[i] != g.start) { printf("starts[%zu] differs\n", i); rc = 3; }
        }
        printf("order");
        for (uint32_t i : plan.order) printf(" %u", i);
        printf("\ntotal %llu\n", (unsigned long long)plan.total);
    }
    // a member outside the buffer, by offset and by length, and an offset that would wrap a 64-bit sum
    const GzMemberIn outside[3] = {{bytes.size() + 1, 0, 0}, {0, (uint32_t)bytes.size() + 1u, 0}, {~0ull - 3, 8, 0}};
    for (const GzMemberIn& m : outside) if (gz_plan(packed, bytes.size(), &m, 1, plan, err)) { printf("a member outside the buffer was planned\n"); rc = 3; }
    if (gz_plan(packed, bytes.size(), members.data(), 0, plan, err)) { printf("an empty table was planned\n"); rc = 3; }
    free(packed);
    return rc;
}
