"""CPU: the piece rules of matchy_amd/csrc/inflate_core.h (pieces of one DEFLATE stream), driven sequentially through all passes by
tests/cpp/test_gz_pieces.cpp, compiled with g++ under -fsanitize=address,undefined as a stand-alone program and fed every vector of
tests/gz_pieces_cases.py. This run comes in front of any GPU run of the hostile vectors: a load behind a member's end, or a store outside
a piece's own range of the symbols or outside the text, stops the sanitized program. Also the raised member bound of gz_packer.h and the
split rule of gz_plan.h. No GPU."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

import gz_cases as G
import gz_pieces_cases as P
from test_inflate_core_host import SAN, build

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("gz_pieces"), "test_gz_pieces")


@pytest.fixture(scope="module")
def results(driver, tmp_path_factory):
    """every vector through the driver, once: name -> (status, text, pieces)"""
    tmp = tmp_path_factory.mktemp("gz_pieces_run")
    out = {}
    for k, (name, gz, piece_bytes, _, _) in enumerate(P.cases()):
        (got,) = P.run_driver(driver, tmp, [(gz, 0)], piece_bytes, tag=str(k))
        out[name] = got
    return out


def counts(pieces):
    live = sum(1 for p in pieces if p[5] & P.LIVE)
    dead = sum(1 for p in pieces if p[5] & P.HAS_START and not p[5] & P.LIVE)
    return live, dead


def test_bytes_and_statuses_are_zlibs(results):
    for name, gz, _, status, text in P.cases():
        st, t, pieces = results[name]
        ok, ztext = P.verdict(gz)
        assert (st == "OK") == ok and t == ztext, name
        assert (st, t) == (status, text), name
        live, dead = counts(pieces)
        print(f"{name}: {len(gz)} bytes, {len(pieces)} pieces, {live} live, {dead} dead, handed over {bool(pieces[0][5] & P.HANDED)}")
        assert len(pieces) >= 10, name   # every vector is split


def test_pieces_that_would_hide_a_failure(results):
    """without these the vectors could pass with everything decoded by piece 0 or by the handover"""
    for name, least in (("v1_l6", 8), ("v2_zblock", 16)):
        st, _, pieces = results[name]
        assert st == "OK" and counts(pieces)[0] >= least and not pieces[0][5] & P.HANDED, (name, counts(pieces))
    st, _, pieces = results["v5_false_starts"]
    assert st == "OK" and counts(pieces)[1] >= 1 and not pieces[0][5] & P.HANDED
    st, _, pieces = results["v3_fixed"]
    assert st == "OK" and counts(pieces) == (1, 0) and not pieces[0][5] & P.HANDED
    for name in ("v3_stored_mix", "v4_seam", "v4_run", "v4_short_pieces"):
        st, _, pieces = results[name]
        assert st == "OK" and counts(pieces)[0] >= 8 and not pieces[0][5] & P.HANDED, (name, counts(pieces))
    assert all(p[3] < 32768 for p in results["v4_short_pieces"][2])
    # the dictionary: handed over both ways — in piece 0 the chain breaks at once, in a later piece it is complete and a marker fails
    st, _, pieces = results["v6_dict_piece0"]
    assert st == "BAD_DISTANCE" and pieces[0][5] & P.HANDED and not pieces[0][5] & P.LIVE
    st, _, pieces = results["v6_dict_later"]
    assert st == "BAD_DISTANCE" and pieces[0][5] & P.HANDED and counts(pieces)[0] >= 8


def test_live_pieces_tile_the_stream(results):
    """every live piece starts at the bit where the one in front ended, and out_pos is the running sum"""
    for name, _, _, status, text in P.cases():
        st, _, pieces = results[name]
        live = [p for p in pieces if p[5] & P.LIVE]
        if status != "OK":
            continue
        assert live[0][0] == 0 and live[0][4] == 0
        for a, b in zip(live, live[1:]):
            assert b[0] == a[1] and b[4] == a[4] + a[3], name
        assert live[-1][4] + live[-1][3] == len(text), name


def test_mutants(driver, tmp_path):
    """v7, all of them: zlib decides. Rejected, or not at its end -> a status other than OK, and the one the sequential decoder gives (the
    driver with a piece size no member reaches); accepted -> OK and zlib's bytes."""
    gz, text = P.mutant_source()
    muts = P.mutants()
    verdicts = [P.verdict(m) for m in muts]
    workers = max(1, min(8, os.cpu_count() or 1))
    chunks = [list(range(k, len(muts), workers)) for k in range(workers)]

    def run(k):
        cases = [(muts[i], len(text)) for i in chunks[k]]
        return P.run_driver(driver, tmp_path, cases, P.MUTANT_PIECE_BYTES, tag="p%d" % k), P.run_driver(driver, tmp_path, cases, 1 << 20, tag="s%d" % k)
    with ThreadPoolExecutor(workers) as pool:
        done = list(pool.map(run, range(workers)))
    split = handed = 0
    for k, (with_pieces, without) in enumerate(done):
        for i, (st, out, pieces), (st0, out0, pieces0) in zip(chunks[k], with_pieces, without):
            ok, t = verdicts[i]
            assert not pieces0
            if ok:
                assert st == "OK" and out == t, i
            else:
                assert st != "OK" and st == st0, (i, st, st0)
            split += bool(pieces)
            handed += bool(pieces and pieces[0][5] & P.HANDED)
    print(f"{len(muts)} mutants, {sum(ok for ok, _ in verdicts)} accepted, {split} split, {handed} handed over")
    assert split * 10 >= len(muts) * 9 and handed < split   # the shortest prefixes are not split; an accepted mutant is not handed over
    (st, out, pieces), = P.run_driver(driver, tmp_path, [(gz, len(text))], P.MUTANT_PIECE_BYTES, tag="pristine")
    assert (st, out) == ("OK", text) and counts(pieces)[0] >= 4


def test_split_rule_and_scratch_bound(tmp_path):
    """gz_plan.h gz_plan_pieces: body_len >= 2 * piece_bytes, valid sizes, first_piece in table order, the scratch bound"""
    exe = tmp_path / "plan_pieces"
    src = tmp_path / "plan_pieces.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include "gz_plan.h"
using namespace mxy;
int main(int argc, char** argv) {   // PIECE_BYTES then body_len:cap ...
    const uint32_t pb = (uint32_t)strtoul(argv[1], nullptr, 10);
    std::vector<GzPlanned> m;
    std::vector<uint32_t> order;
    for (int i = 2; i < argc; ++i) { unsigned long long b, c; sscanf(argv[i], "%llu:%llu", &b, &c); m.push_back(GzPlanned{0, (uint32_t)b, 0, (uint32_t)c, GZ_PLAN_OK}); order.push_back((uint32_t)(i - 2)); }
    GzPiecePlan pp;
    gz_plan_pieces(m, order, pb, pp);
    printf("valid %d split", (int)gz_piece_bytes_valid(pb));
    for (uint32_t s : pp.split) printf(" %u", s);
    printf("\nfirst");
    for (uint32_t f : pp.first_piece) printf(" %u", f);
    printf("\norder");
    for (uint32_t o : order) printf(" %u", o);
    printf("\nscratch %llu\n", (unsigned long long)pp.scratch_syms);
}''')
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(src), "-o", str(exe)], check=True)

    def plan(pb, *members):
        r = subprocess.run([str(exe), str(pb), *["%d:%d" % m for m in members]], capture_output=True, text=True, check=True)
        return [ln.split()[1:] for ln in r.stdout.splitlines()]
    assert plan(1024, (2047, 9000), (2048, 9000), (5000, 0), (4097, 70000)) == [["1", "split", "1", "3"], ["0", "0", "2", "2", "7"], ["0", "2"], ["79000"]]
    for bad in (0, 3, 256, 768, 1 << 21):
        assert plan(bad, (1 << 22, 1 << 22))[0][:2] == ["0", "split"] and plan(bad, (1 << 22, 1 << 22))[2] == ["0"]
    # 4 GiB of scratch: 2 bytes per byte of capacity, in claim order; what does not fit stays unsplit
    half = 1 << 30
    assert plan(4096, (1 << 20, half), (1 << 20, half), (1 << 20, 1))[0] == ["1", "split", "0", "1"]
    assert plan(4096, (1 << 20, half + 1), (1 << 20, half), (1 << 20, 1))[0] == ["1", "split", "0", "2"]


def test_packer_member_bound_with_pieces(tmp_path):
    """gz_packer.h gz_bounds_pieces: the member bound is what a pack can hold, the overrides lower it, gz_bounds is as it was"""
    exe = tmp_path / "bounds_pieces"
    src = tmp_path / "bounds_pieces.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include "gz_packer.h"
using namespace mxy;
int main(int argc, char** argv) {   // BATCH MAX_MEMBER|- MAX_CARRY|- ISIZE
    auto opt = [](const char* s) { return strcmp(s, "-") ? std::optional<uint64_t>(strtoull(s, nullptr, 10)) : std::nullopt; };
    const GzBounds p = gz_bounds_pieces(strtoull(argv[1], nullptr, 10), opt(argv[2]), opt(argv[3])), b = gz_bounds(strtoull(argv[1], nullptr, 10), opt(argv[2]), opt(argv[3]));
    uint8_t file[20] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3, 3, 0};
    const uint32_t isize = (uint32_t)strtoull(argv[4], nullptr, 10);
    memcpy(file + 16, &isize, 4);
    std::vector<uint64_t> cuts;
    uint32_t n = 0, is = 0;
    printf("%zu %zu %zu %llu | %zu %zu %zu %llu | %d %d\n", p.batch_bytes, p.max_member, p.carry_cap, (unsigned long long)p.max_text, b.batch_bytes, b.max_member, b.carry_cap,
           (unsigned long long)b.max_text, (int)gz_eligible_bytes(file, 20, p, false, cuts, n, is), (int)gz_eligible_bytes(file, 20, b, false, cuts, n, is));
}''')
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(src), "-o", str(exe)], check=True)

    def bounds(bb, mm, cc, isize):
        r = subprocess.run([str(exe), str(bb), "-" if mm is None else str(mm), "-" if cc is None else str(cc), str(isize)], capture_output=True, text=True, check=True)
        p, b, e = r.stdout.split("|")
        return tuple(map(int, p.split())), tuple(map(int, b.split())), tuple(map(int, e.split()))
    bb = 1 << 28
    p, b, e = bounds(bb, None, None, bb // 4 + 1)
    assert b == (bb, bb // 4, 1 << 20, bb - (1 << 20)) and p == (bb, bb - (1 << 20), 1 << 20, bb - (1 << 20))
    assert e == (1, 0)                                               # one byte above a quarter of a batch: with pieces only
    assert bounds(bb, None, None, bb - (1 << 20))[2] == (1, 0) and bounds(bb, None, None, bb - (1 << 20) + 1)[2] == (0, 0)
    assert bounds(bb, 5000, None, 5001)[0][1] == 5000 and bounds(bb, 5000, None, 5001)[2] == (0, 0)   # the override lowers it
    assert bounds(bb, None, 0, bb - 1)[0][1:] == (bb - 1, 0, bb) and bounds(bb, None, 0, bb - 1)[2][0] == 1   # the separator still fits
    assert bounds(bb, None, 0, bb)[2][0] == 0
    assert bounds(1 << 40, None, None, 1)[0][0] == (1 << 31) - (1 << 20)
