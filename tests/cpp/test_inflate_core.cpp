// CPU: the decoder rules of k_gz_inflate (matchy_amd/csrc/inflate_core.h) driven sequentially, the way the wave drives them: lane 0's
// decode_batch into a queue of 64 tokens, the queue executed (literals, then the matches in order, then the stored run), the CRC-32 as
// 64 lane parts, the trailer check. Built with -fsanitize=address,undefined (tests/test_inflate_core_host.py): every member is copied
// into a heap block of exactly its length and inflated into a heap block of exactly its capacity, so a load behind the member's end
// or a store behind its capacity stops the run.
//
//   test_inflate_core CASES OUT     CASES: u32 n, then per case u32 len, u32 out_len, bytes (tests/gz_cases.py)
//                                   OUT:   per case i32 status, u32 n, n bytes (the text of an OK member; n = 0 otherwise)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gz_plan.h"
#include "inflate_core.h"

using namespace mxy;

static int32_t inflate_member(const uint8_t* body, uint32_t body_len, uint8_t* out, uint32_t cap, gz::Tables& tab, const uint32_t* crc_tab) {
    gz::Decoder d;
    gz::decoder_init(d, body, body_len, cap);
    gz::Token queue[64];
    gz::Batch batch;
    for (uint64_t turns = 8ull * body_len + 2ull; turns; --turns) {
        gz::decode_batch(d, tab, queue, 64, batch);
        for (uint32_t k = 0; k < batch.n; ++k) if (!gz::token_is_match(queue[k])) out[queue[k].pos] = (uint8_t)queue[k].v;
        for (uint32_t k = 0; k < batch.n; ++k) {
            if (!gz::token_is_match(queue[k])) continue;
            const uint32_t len = gz::token_len(queue[k]), dist = gz::token_dist(queue[k]), pos = queue[k].pos;
            // a wave copies 64 bytes at a time and reads all of them first: sources in front of pos make that the same as this loop
            for (uint32_t i = 0; i < len; ++i) {
                if (gz::match_src(pos, dist, i) >= pos) { fprintf(stderr, "match source at or behind its position\n"); exit(3); }
                out[pos + i] = out[gz::match_src(pos, dist, i)];
            }
        }
        for (uint32_t i = 0; i < batch.stored_len; ++i) out[batch.stored_pos + i] = body[batch.stored_src + i];
        if (d.done || d.status != gz::GZ_OK) break;
    }
    if (d.status != gz::GZ_OK) return d.status;
    if (!d.done) return gz::GZ_TRUNCATED;
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) crc ^= gz::crc_lane_part(crc_tab, out, d.produced, lane, 64);
    return gz::check_trailer(d, crc);
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: test_inflate_core CASES OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    FILE* o = fopen(argv[2], "wb");
    if (!f || !o) { perror("open"); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    uint32_t crc_tab[256];
    for (uint32_t i = 0; i < 256; ++i) crc_tab[i] = gz::crc_table_entry(i);
    gz::Tables* tab = new gz::Tables();
    size_t ok = 0;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t hdr[2];
        if (fread(hdr, 4, 2, f) != 2) return 2;
        uint8_t* file = (uint8_t*)malloc(hdr[0] ? hdr[0] : 1);   // exactly the member: the sanitizer sees a load behind it
        if (hdr[0] && fread(file, 1, hdr[0], f) != hdr[0]) return 2;
        const GzMemberIn m{0, hdr[0], hdr[1]};
        GzPlan plan;
        std::string err;
        if (!gz_plan(file, hdr[0], &m, 1, plan, err)) { fprintf(stderr, "case %u: %s\n", c, err.c_str()); return 2; }
        const GzPlanned& g = plan.members[0];
        int32_t status = g.status;
        uint8_t* out = (uint8_t*)malloc(g.cap ? g.cap : 1);      // exactly the capacity
        if (status == gz::GZ_OK) status = inflate_member(file + g.body, g.body_len, out, g.cap, *tab, crc_tab);
        const uint32_t len = status == gz::GZ_OK ? g.cap : 0u;
        fwrite(&status, 4, 1, o);
        fwrite(&len, 4, 1, o);
        if (len) fwrite(out, 1, len, o);
        ok += status == gz::GZ_OK;
        free(out);
        free(file);
    }
    delete tab;
    fclose(f);
    if (fclose(o) != 0) return 2;
    printf("inflate_core ok: %u cases, %zu inflated\n", n, ok);
    return 0;
}
