// CPU: the window walker and the window plan of a gz scan (matchy_amd/csrc/gz_plan.h: gz_next_window, gz_plan_window) printed for
// tests/test_gz_window_host.py to hold against its model. Built with -fsanitize=address,undefined; every input lies in a heap block of
// exactly its length, so a read behind a file's end stops the program.
//
//   test_gz_window walk CASES MAX_COMP MAX_TEXT MAX_MEMBER
//                                CASES: u32 n, then per case u32 len, u32 (unused), bytes — one FILE per case
//                                prints per file "window i end members text c0 c1 ..." for every window (c: where its members start) and
//                                "stop i from" where the walker yields no window; the cuts of all windows are held against
//                                gz_split_members here as well (exit 3 where they differ)
//   test_gz_window plan CASES CARRY_LEN LAST
//                                the cases, end to end, are the members of ONE window
//                                prints "member i body body_len start cap status", "window first start cap", "total N";
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
    const bool walk = argc == 6 && !strcmp(argv[1], "walk"), plan_mode = argc == 5 && !strcmp(argv[1], "plan");
    if (!walk && !plan_mode) { fprintf(stderr, "usage: test_gz_window walk CASES MAX_COMP MAX_TEXT MAX_MEMBER | plan CASES CARRY_LEN LAST\n"); return 2; }
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
    if (walk) {
        const uint64_t max_comp = strtoull(argv[3], nullptr, 10), max_text = strtoull(argv[4], nullptr, 10), max_member = strtoull(argv[5], nullptr, 10);
        std::vector<uint64_t> cuts, all, whole;
        for (uint32_t c = 0; c < n; ++c) {
            const size_t len = cases[c].size();
            uint8_t* p = (uint8_t*)malloc(len ? len : 1);
            if (len) memcpy(p, cases[c].data(), len);
            all.clear();
            uint64_t from = 0;
            GzWindow w;
            for (;;) {
                cuts.clear();
                if (!gz_next_window(p, len, from, max_comp, max_text, max_member, w, &cuts)) break;
                printf("window %u %llu %u %llu", c, (unsigned long long)w.end, w.members, (unsigned long long)w.text);
                for (uint64_t q : cuts) printf(" %llu", (unsigned long long)q);
                printf("\n");
                if (w.members == 0 || cuts.size() != w.members || cuts[0] != from || w.end <= from || w.end > len || w.end - from > max_comp || w.text > max_text) {
                    printf("file %u: a window breaks its rules\n", c); rc = 3; break;
                }
                all.insert(all.end(), cuts.begin(), cuts.end());
                from = w.end;
            }
            if (w.end != from || w.members != 0) { printf("file %u: no window, but an end or a member count\n", c); rc = 3; }
            printf("stop %u %llu\n", c, (unsigned long long)from);
            gz_split_members(p, len, whole);
            if (from == len && len) {   // walked to the end: the same cuts as the split of the whole file
                if (all != whole) { printf("file %u: the windows' cuts are not those of gz_split_members\n", c); rc = 3; }
            } else if (all.size() > whole.size() || !std::equal(all.begin(), all.end(), whole.begin())) { printf("file %u: the windows' cuts are no prefix of gz_split_members\n", c); rc = 3; }
            free(p);
        }
        return rc;
    }
    const uint32_t carry_len = (uint32_t)strtoull(argv[3], nullptr, 10);
    const bool last = atoi(argv[4]) != 0;
    size_t total = 0;
    for (const auto& c : cases) total += c.size();
    uint8_t* packed = (uint8_t*)malloc(total ? total : 1);
    size_t at = 0;
    for (const auto& c : cases) { if (!c.empty()) memcpy(packed + at, c.data(), c.size()); at += c.size(); }
    GzFilesPlan plan;
    std::string err;
    if (!gz_plan_window(packed, total, carry_len, last, plan, err)) { printf("refused: %s\n", err.c_str()); rc = 1; }
    else {
        for (size_t i = 0; i < plan.members.size(); ++i) {
            const GzPlanned& g = plan.members[i];
            printf("member %zu %llu %u %u %u %d\n", i, (unsigned long long)g.body, g.body_len, g.start, g.cap, g.status);
        }
        printf("window %u %u %u\n", plan.first_member[0], plan.starts[0], plan.caps[0]);
        if (plan.starts.size() != 1 || plan.first_member.size() != 2 || plan.first_member[1] != plan.members.size()) { printf("not one segment\n"); rc = 3; }
        printf("total %llu\n", (unsigned long long)plan.total);
    }
    free(packed);
    return rc;
}
