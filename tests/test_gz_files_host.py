"""CPU: the host side of gz scans of multi-member files — the member split and the file plan (matchy_amd/csrc/gz_plan.h: gz_split_members,
gz_plan_files), compiled with g++ under -fsanitize=address,undefined as a stand-alone program and held against the Python model of
tests/gz_files_cases.py; and the C ABI surface of the new calls. This run comes in front of any GPU run of the corrupt vectors. No GPU."""
import ctypes as C
import gzip
import re
import struct
import subprocess
from pathlib import Path

import pytest

import gz_cases as G
import gz_files_cases as F

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
INVALID = -5
NEW_FUNCTIONS = ("matchy_scanner_scan_gz_files", "matchy_scan_result_gz_files", "matchy_multi_scanner_submit_gz_files")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gz_split") / "test_gz_split"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "test_gz_split.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def split(driver, tmp_path, files):
    src = tmp_path / "files.bin"
    G.write_case_file(src, [(f, 0) for f in files])
    r = subprocess.run([str(driver), "split", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    rows = [list(map(int, ln.split()[2:])) for ln in r.stdout.splitlines() if ln.startswith("file ")]
    assert len(rows) == len(files)
    return rows


def plan(driver, tmp_path, files):
    src = tmp_path / "pack.bin"
    G.write_case_file(src, [(f, 0) for f in files])
    return subprocess.run([str(driver), "plan", str(src)], capture_output=True, text=True)


def test_random_concatenations_are_cut_at_the_true_members(driver, tmp_path):
    """200 concatenations of 1-9 members, 0-60 lines each, levels 0-9, with and without a final newline: the cuts are exactly the true
    ones, the model agrees, and zlib reads the same text"""
    cases = [F.rand_concat(seed) for seed in range(200)]
    got = split(driver, tmp_path, [f for f, _, _ in cases])
    assert sum(len(c) for _, c, _ in cases) > 600
    for seed, ((f, cuts, text), row) in enumerate(zip(cases, got)):
        assert row == cuts, seed
        assert F.split_members(f) == cuts, seed
        assert gzip.decompress(f) == text, seed


def test_a_large_single_member_log_yields_no_false_cut(driver, tmp_path):
    text = G.log(48000, seed=77)
    assert len(text) > 6_000_000
    f = F.member(text)
    assert split(driver, tmp_path, [f]) == [[0]] and F.split_members(f) == [0]


def test_header_variants_bgzf_and_hostile_files(driver, tmp_path):
    """later members with FNAME / FCOMMENT / FEXTRA / FHCRC; BGZF with the empty end block; BSIZE that points outside the file or at
    no header; the stored member that holds a .gz file; 1 000 header patterns; every proper prefix of a three-member file"""
    good = {name: f for name, f, _ in F.good_files()}
    t = [G.log(3, seed=k) for k in (5, 6, 7)]
    later = good["later_headers"]
    bgzf = good["bgzf"]
    outside = F.bgzf_member(t[0], bsize=60000) + F.bgzf_member(t[1])
    lying = dict((n, f) for n, f, _ in F.reject_files())["lying_bsize"]
    stored = F.stored_false_cut()
    three = F.member(t[0]) + F.member(t[1], 9) + F.member(t[2], 1)
    files = [later, bgzf, outside, lying, stored, F.header_patterns(), F.header_patterns(os_byte=3), b"", b"\x1f", F.BGZF_EOF] + [three[:n] for n in range(len(three))]
    got = split(driver, tmp_path, files)
    for f, row in zip(files, got):
        assert row == F.split_members(f), len(f)
    assert len(got[0]) == 6                                  # every later header is found
    n_blocks = -(-len(gzip.decompress(bgzf)) // 997)
    assert len(got[1]) == n_blocks + 1                       # the 28-byte end block is a member of its own
    assert got[2] == [0] and got[3] == [0]                   # a lying BSIZE: the member keeps the rest of the file
    assert got[4] == [0, 20]                                 # the false cut at the embedded header
    assert got[5] == list(range(0, 10000, 20))               # one header parse per pattern, pieces of 20 bytes
    assert got[9] == [0]
    true_cuts = F.split_members(three)
    assert len(true_cuts) == 3
    for n in range(len(three)):                              # a prefix is cut where the whole file is, as far as a header fits
        assert got[10 + n] == [c for c in true_cuts if c == 0 or F.parse_header(three[:n], c) is not None], n


def parse_plan(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    members = [list(map(int, ln.split()[2:])) for ln in out if ln.startswith("member ")]
    files = [list(map(int, ln.split()[2:])) for ln in out if ln.startswith("file ")]
    order = [int(x) for ln in out if ln.startswith("order") for x in ln.split()[1:]]
    total = [int(ln.split()[1]) for ln in out if ln.startswith("total ")][0]
    return members, files, order, total


def test_file_plan_against_the_model(driver, tmp_path):
    """starts, nothing between the members of a file and one separator behind it, files whose members are all empty, members the plan
    refuses, and the claim order over the members of all files"""
    files = [f for _, f, _ in F.good_files()] + [f for _, f, _ in F.reject_files()] + [b"", b"\x1f\x8b", F.member(b"abc")[:14]]
    members, rows, order, total = parse_plan(plan(driver, tmp_path, files))
    want_members, first, starts, caps, want_total = F.plan_files(files)
    assert [(m[0], m[5], m[4], m[3]) for m in members] == want_members
    assert [tuple(r) for r in rows] == list(zip(first[:-1], starts, caps)) and total == want_total
    for f, (fm, st, cap) in enumerate(rows):                 # the layout rule, spelled out
        mine = [m for m in members if m[0] == f]
        assert mine[0][3] == st and all(b[3] == a[3] + a[4] for a, b in zip(mine, mine[1:])) and sum(m[4] for m in mine) == cap
        if f + 1 < len(rows):
            assert rows[f + 1][1] == st + cap + (1 if cap else 0)
    names = [n for n, _, _ in F.good_files()]
    assert caps[names.index("only_empty")] == 0 and rows[names.index("only_empty")][0] + 3 == rows[names.index("only_empty") + 1][0]
    offset = 0
    for f, b in enumerate(files):                            # body / body_len of every member the plan accepts
        cuts = F.split_members(b)
        for k, m in enumerate(m for m in members if m[0] == f):
            piece = b[cuts[k]:cuts[k + 1] if k + 1 < len(cuts) else len(b)]
            if m[5] == 0:
                hl = G.header_len(piece)
                assert (m[1], m[2]) == (offset + cuts[k] + hl, len(piece) - hl), (f, k)
        offset += len(b)
    ok = [i for i, m in enumerate(members) if m[5] == 0]
    assert order == sorted(ok, key=lambda i: (-members[i][4], i)) and len(ok) < len(members)


def test_hostile_fname_patterns_cost_linear_time(driver, tmp_path):
    """1 MiB of header patterns with the FNAME bit and no zero byte behind them: every pattern is a candidate, none is a cut, and a
    candidate reads at most GZ_SPLIT_MAX_STR bytes of name. A parse that ran to the end of the file for every pattern took minutes
    here (512 KiB: 6 s without the sanitizer); the bound is 100 000 candidates of 256 bytes, tens of milliseconds. A later member
    whose name has 255 bytes is found, one with 256 is not."""
    import time
    hostile = F.fname_patterns()
    assert len(hostile) > 1 << 20 and b"\0" not in hostile[10:]
    t = G.log(3, seed=8)
    fits = F.member(t) + F.member(t, flg=8, name=b"n" * 255)
    too_long = F.member(t) + F.member(t, flg=8, name=b"n" * 256)
    t0 = time.perf_counter()
    got = split(driver, tmp_path, [hostile, fits, too_long])
    took = time.perf_counter() - t0
    assert got[0] == [0] == F.split_members(hostile)
    assert got[1] == [0, len(F.member(t))] == F.split_members(fits) and got[2] == [0] == F.split_members(too_long)
    assert took < 2.0, took
    r = plan(driver, tmp_path, [hostile, fits])
    assert r.returncode == 0 and "file 1 1 " in r.stdout, r.stdout[-500:] + r.stderr[-2000:]


def test_file_plan_refusals(driver, tmp_path):
    """a batch that reaches 2^31 bytes is refused, one byte less per file is not; ISIZE fields of 0xFFFFFFFF are summed in 64 bits"""
    body = G.raw_deflate(b"x")

    def vouch(isize):
        return G.gz_wrap(body, b"x", isize=isize)
    r = plan(driver, tmp_path, [vouch((1 << 30) - 1)] * 2)
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, [vouch((1 << 30) - 2)] * 2)
    assert r.returncode == 0 and "total %d\n" % ((1 << 31) - 2) in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, [vouch((1 << 30) - 1) + vouch((1 << 30) - 1)])   # one file of two members: no separator between them
    assert r.returncode == 0 and "total %d\n" % ((1 << 31) - 1) in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, [vouch((1 << 30) - 1) + vouch(1 << 30)])
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, [vouch(0xFFFFFFFF) * 3, vouch(0xFFFFFFFF)])
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, [F.header_patterns(os_byte=3)])                  # 500 pieces that vouch for 48 MiB each
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr


def test_header_export_list_library_and_mirror_carry_the_new_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct matchy_gz_file_t \{ uint64_t offset; uint64_t len; \} matchy_gz_file_t;", header)
    assert C.sizeof(M._GzFile) == 16 and M._GzFile.len.offset == 8
    assert re.search(r"matchy_scanner_scan_gz_files\s*\(\s*matchy_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const matchy_gz_file_t\s*\*\s*\w+,"
                     r"\s*size_t\s+\w+,\s*uint32_t\s+\w+,\s*bool\s+\w+,\s*matchy_scan_result_t\s*\*\s*\w+\)", header)
    assert re.search(r"matchy_scan_result_gz_files\s*\(\s*const matchy_scan_result_t\s*\*\s*\w+,\s*const int32_t\s*\*\*\s*\w+,\s*size_t\s*\*\s*\w+,\s*const uint32_t\s*\*\*\s*\w+\)", header)
    assert re.search(r"matchy_multi_scanner_submit_gz_files\s*\(\s*matchy_multi_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const matchy_gz_file_t\s*\*\s*\w+,"
                     r"\s*size_t\s+\w+,\s*bool\s+\w+,\s*void\s*\*\s*\w+\)", header)
    for cls, attrs in ((M.Scanner, ("scan_gz_files",)), (M.MultiScanner, ("submit_gz_files_ptr",)), (M.ScanResult, ("gz_file_status", "gz_first_member"))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)
    assert M.GZ_STATUS_NAMES == G.STATUS and len(re.findall(r"#define MATCHY_GZ_[A-Z_]+ \d+", header)) == 11   # no new status value


def test_null_handles_and_empty_tables_are_refused():
    import matchy_amd as M
    L = M.lib()
    raw = M._ScanResult()
    table = (M._GzFile * 1)()
    assert L.matchy_scanner_scan_gz_files(None, None, 0, None, 0, 1, False, None) == INVALID
    assert L.matchy_scanner_scan_gz_files(None, b"x", 1, table, 1, 1, False, C.byref(raw)) == INVALID
    assert L.matchy_scan_result_gz_files(None, None, None, None) == INVALID
    assert L.matchy_scan_result_gz_files(C.byref(raw), None, None, None) == INVALID and "gz scan" in M.last_error()
    assert L.matchy_multi_scanner_submit_gz_files(None, None, 0, None, 0, False, None) == INVALID


def test_sources():
    hip = (ROOT / "matchy_amd" / "csrc" / "inflate.hip").read_text()
    for k in ("k_gz_inflate", "k_gz_seal", "k_gz_file_verdict", "k_gz_seal_files"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    import matchy_amd.build as B
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--gz-members" in src and "matchy_multi_scanner_submit_gz_files" in src
    assert "hip/" not in (ROOT / "matchy_amd" / "csrc" / "gz_plan.h").read_text()
    assert struct.calcsize("<QQ") == 16
