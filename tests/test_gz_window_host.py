"""CPU: the host side of gz windows — the incremental member walker and the window plan (matchy_amd/csrc/gz_plan.h: gz_next_window,
gz_plan_window), compiled with g++ under -fsanitize=address,undefined as a stand-alone program and held against the Python models of
tests/gz_window_cases.py; and the C ABI surface of the new calls. No GPU."""
import ctypes as C
import re
import subprocess
import time
from pathlib import Path

import pytest

import gz_cases as G
import gz_files_cases as F
import gz_window_cases as W

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
INVALID = -5
NEW_FUNCTIONS = ("matchy_scanner_scan_gz_window", "matchy_scan_result_gz_window", "matchy_multi_scanner_submit_gz_window")
HUGE = 1 << 40


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gz_window") / "test_gz_window"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "test_gz_window.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def walk(driver, tmp_path, files, max_comp, max_text, max_member):
    """[([(end, members, text, [cuts])], stop)] per file, as the program prints them"""
    src = tmp_path / "files.bin"
    G.write_case_file(src, [(f, 0) for f in files])
    r = subprocess.run([str(driver), "walk", str(src), str(max_comp), str(max_text), str(max_member)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    out = [([], None) for _ in files]
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "window":
            v = list(map(int, w[1:]))
            out[v[0]][0].append((v[1], v[2], v[3], v[4:]))
        elif w[0] == "stop":
            out[int(w[1])] = (out[int(w[1])][0], int(w[2]))
    assert all(stop is not None for _, stop in out)
    return out


def plan(driver, tmp_path, members, carry_len, last):
    src = tmp_path / "window.bin"
    G.write_case_file(src, [(m, 0) for m in members])
    return subprocess.run([str(driver), "plan", str(src), str(carry_len), str(int(last))], capture_output=True, text=True)


def test_the_walker_yields_the_cuts_of_the_split(driver, tmp_path):
    """the 200 random concatenations and the good files under bounds small enough that most files take three windows or more: the
    windows' cuts, concatenated, are those of gz_split_members (held in the program) and of the model; every window holds a member
    and keeps both bounds; the walker agrees with its model window for window"""
    cases = [F.rand_concat(seed) for seed in range(200)]
    files = [f for f, _, _ in cases] + [f for _, f, _ in F.good_files()]
    max_comp, max_text, max_member = 8000, 8000, HUGE
    got = walk(driver, tmp_path, files, max_comp, max_text, max_member)
    whole, many = 0, 0
    for k, (f, (windows, stop)) in enumerate(zip(files, got)):
        assert (windows, stop) == W.walk_windows(f, max_comp, max_text, max_member), k
        at = 0
        for end, members, text, cuts in windows:
            assert members >= 1 and len(cuts) == members and cuts[0] == at and end - at <= max_comp and text <= max_text, k
            at = end
        cuts = [c for _, _, _, cs in windows for c in cs]
        true = F.split_members(f)
        assert cuts == true[:len(cuts)], k
        if stop == len(f):
            assert cuts == true, k
            whole += 1
            many += len(windows) >= 3
    assert whole == len(files) and many > whole // 2, (whole, many)
    got = walk(driver, tmp_path, files, HUGE, HUGE, HUGE)        # without bounds: one window, the true cuts
    for k, (f, (windows, stop)) in enumerate(zip(files, got)):
        assert stop == len(f) and len(windows) == 1 and windows[0][3] == F.split_members(f), k
    for (f, true, _), (windows, _) in zip(cases, got):
        assert windows[0][3] == true


def test_every_prefix_of_a_three_member_file_is_walked_inside_its_bytes(driver, tmp_path):
    """the sanitizer stops a read behind a prefix's end; the walker and the model agree on every prefix, with and without bounds"""
    t = [G.log(3, seed=k) for k in (5, 6, 7)]
    three = F.member(t[0]) + F.member(t[1], 9) + F.member(t[2], 1)
    prefixes = [three[:n] for n in range(len(three) + 1)]
    for bounds in ((len(F.member(t[0])) + 5, HUGE, HUGE), (HUGE, len(t[0]) + 1, HUGE), (HUGE, HUGE, HUGE)):
        got = walk(driver, tmp_path, prefixes, *bounds)
        for n, (p, g) in enumerate(zip(prefixes, got)):
            assert g == W.walk_windows(p, *bounds), (n, bounds)
    assert got[len(three)] == ([(len(three), 3, sum(map(len, t)), F.split_members(three))], len(three))
    assert got[0] == ([], 0) and got[5] == ([], 0)


def test_an_oversized_member_stops_the_walk_exactly_there(driver, tmp_path):
    """a member whose compressed length, or whose ISIZE, is above max_member in the middle of a file: windows up to it, then none; a
    member without room for its trailer, and bytes that are no header, likewise"""
    small = [G.log(2, seed=30 + k) for k in range(6)]
    big = G.log(60, seed=40)
    ms = [F.member(x) for x in small]
    big_m = F.member(big)
    f = ms[0] + ms[1] + ms[2] + big_m + ms[3] + ms[4]
    at = len(ms[0] + ms[1] + ms[2])
    assert len(big_m) > 1000 > max(len(m) for m in ms) and len(big) > 1000
    for bounds in ((HUGE, HUGE, 1000), (HUGE, HUGE, len(big) - 1), (1000, HUGE, HUGE), (HUGE, len(big) - 1, HUGE)):
        (windows, stop), = walk(driver, tmp_path, [f], *bounds)
        assert stop == at and sum(w[1] for w in windows) == 3, bounds
    (windows, stop), = walk(driver, tmp_path, [f], HUGE, HUGE, len(big))         # both of its lengths fit: the walk goes through
    assert stop == len(f) and sum(w[1] for w in windows) == 6
    vouch = G.gz_wrap(G.raw_deflate(b"x"), b"x", isize=0xFFFFFFFF)                # an ISIZE that only a 64-bit sum holds
    (windows, stop), = walk(driver, tmp_path, [ms[0] + vouch * 3 + ms[1]], HUGE, (1 << 32) + 1000, HUGE)
    assert [w[1] for w in windows] == [2, 1, 2] and [w[2] for w in windows] == [0xFFFFFFFF + len(small[0]), 0xFFFFFFFF, 0xFFFFFFFF + len(small[1])] and stop == len(ms[0] + vouch * 3 + ms[1])
    garbage = ms[0] + ms[1] + bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3]) + b"\0" * 3   # a header, and no room for a trailer behind it
    (windows, stop), = walk(driver, tmp_path, [garbage], 1 << 20, 1 << 20, 1 << 20)
    assert (windows, stop) == W.walk_windows(garbage, 1 << 20, 1 << 20, 1 << 20) and stop == len(ms[0] + ms[1])
    assert walk(driver, tmp_path, [b"not a gzip file, whatever its name says"], HUGE, HUGE, HUGE) == [([], 0)]


def test_hostile_fname_patterns_are_walked_in_linear_time(driver, tmp_path):
    """the 1 MiB of header patterns with the FNAME bit and no zero byte behind them, within the bound of the split's own test"""
    hostile = F.fname_patterns()
    assert len(hostile) > 1 << 20
    t0 = time.perf_counter()
    got = walk(driver, tmp_path, [hostile, hostile], 1 << 16, 1 << 16, 1 << 16)
    took = time.perf_counter() - t0
    assert got[0] == W.walk_windows(hostile, 1 << 16, 1 << 16, 1 << 16) == ([], 0)   # one member of 1 MiB: above max_member
    assert took < 2.0, took
    got = walk(driver, tmp_path, [hostile], HUGE, HUGE, HUGE)
    assert got[0][1] == len(hostile) and got[0][0][0][3] == [0]


def parse_plan(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    members = [list(map(int, ln.split()[2:])) for ln in out if ln.startswith("member ")]
    window = [list(map(int, ln.split()[1:])) for ln in out if ln.startswith("window ")][0]
    total = [int(ln.split()[1]) for ln in out if ln.startswith("total ")][0]
    return members, window, total


def test_window_plan_against_the_model(driver, tmp_path):
    """the members' starts are shifted by the carry; the window is one segment at 0; the separator only with LAST and a non-empty text"""
    t = [G.log(1 + k, seed=90 + k, final_newline=k % 2 == 0) for k in range(4)]
    shapes = [[F.member(x) for x in t], [F.member(b""), F.member(t[0]), F.member(b"")], [F.member(b""), F.member(b"")],
              F.pieces(F.good_files()[3][1])[:5], [F.member(t[1]), F.member(t[2])[:14]]]
    for members in shapes:
        for carry_len in (0, 1, 77):
            for last in (False, True):
                got_members, window, total = parse_plan(plan(driver, tmp_path, members, carry_len, last))
                want_members, caps, want_total = W.plan_window(b"".join(members), carry_len, last)
                assert [(m[4], m[3], m[2]) for m in got_members] == want_members
                assert window == [0, 0, caps] and total == want_total
                text = carry_len + caps
                assert total == text + (1 if last and text else 0)
                assert got_members[0][2] == carry_len and all(b[2] == a[2] + a[3] for a, b in zip(got_members, got_members[1:]))
    _, _, total = parse_plan(plan(driver, tmp_path, [F.member(b""), F.member(b"")], 0, True))
    assert total == 0                                         # an empty LAST window with an empty carry: no separator
    _, _, total = parse_plan(plan(driver, tmp_path, [F.member(b"")], 5, True))
    assert total == 6


def test_window_plan_refusals(driver, tmp_path):
    """a batch that reaches 2^31 bytes with the carry counted in is refused, one byte below is not"""
    body = G.raw_deflate(b"x")

    def vouch(isize):
        return G.gz_wrap(body, b"x", isize=isize)
    two = [vouch((1 << 30) - 1), vouch((1 << 30) - 1)]        # 2^31 - 2 of text
    r = plan(driver, tmp_path, two, 0, False)
    assert r.returncode == 0 and "total %d\n" % ((1 << 31) - 2) in r.stdout, r.stdout + r.stderr
    r = plan(driver, tmp_path, two, 1, False)
    assert r.returncode == 1 and "2^31" in r.stdout and "carry" in r.stdout, r.stdout + r.stderr
    one = [vouch((1 << 30))]
    r = plan(driver, tmp_path, one, (1 << 30) - 2, True)      # carry + text + separator = 2^31 - 1
    assert r.returncode == 0 and "total %d\n" % ((1 << 31) - 1) in r.stdout, r.stdout + r.stderr
    assert W.plan_window(b"".join(one), (1 << 30) - 2, True)[2] == (1 << 31) - 1
    r = plan(driver, tmp_path, one, (1 << 30) - 1, True)
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
    assert W.plan_window(b"".join(one), (1 << 30) - 1, True) is None and W.plan_window(b"".join(two), 1, False) is None
    r = plan(driver, tmp_path, [vouch(0xFFFFFFFF)] * 3, 0, False)
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr


def test_header_export_list_library_and_mirror_carry_the_new_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert "matchy_scanner_get_gz_window_timing" in M.EXPORTED_SYMBOLS and L.matchy_scanner_get_gz_window_timing is not None
    assert re.search(r"typedef struct matchy_gz_window_t \{ const uint8_t \*carry; uint32_t carry_len, carry_cap, flags; \} matchy_gz_window_t;", header)
    assert C.sizeof(M._GzWindow) == 24 and M._GzWindow.carry_len.offset == 8 and M._GzWindow.carry_cap.offset == 12 and M._GzWindow.flags.offset == 16
    assert re.search(r"matchy_scanner_scan_gz_window\s*\(\s*matchy_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const matchy_gz_window_t\s*\*\s*\w+,"
                     r"\s*uint32_t\s+\w+,\s*bool\s+\w+,\s*matchy_scan_result_t\s*\*\s*\w+\)", header)
    assert re.search(r"matchy_scan_result_gz_window\s*\(\s*const matchy_scan_result_t\s*\*\s*\w+,\s*int32_t\s*\*\s*\w+,\s*const uint8_t\s*\*\*\s*\w+,\s*size_t\s*\*\s*\w+\)", header)
    assert re.search(r"matchy_multi_scanner_submit_gz_window\s*\(\s*matchy_multi_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,"
                     r"\s*const matchy_gz_window_t\s*\*\s*\w+,\s*bool\s+\w+,\s*void\s*\*\s*\w+\)", header)
    for name, value in (("LAST", M.WINDOW_LAST), ("OK", M.WINDOW_OK), ("NO_LINE_END", M.WINDOW_NO_LINE_END)):
        assert int(re.search(r"#define MATCHY_WINDOW_%s (\d+)u?\b" % name, header).group(1)) == value, name
    for cls, attrs in ((M.Scanner, ("scan_gz_window",)), (M.MultiScanner, ("submit_gz_window_ptr",)), (M.ScanResult, ("gz_window",))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)
    assert M.GZ_STATUS_NAMES == G.STATUS and len(re.findall(r"#define MATCHY_GZ_[A-Z_]+ \d+", header)) == 11   # the window status is no MATCHY_GZ_* value
    inflate_h = (ROOT / "matchy_amd" / "csrc" / "inflate.h").read_text()
    assert re.search(r"GZ_TAIL_BLOCK = %d\b" % M.GZ_WINDOW_TAIL_BLOCK, inflate_h)


def test_null_handles_and_empty_windows_are_refused():
    import matchy_amd as M
    L = M.lib()
    raw = M._ScanResult()
    w = M._GzWindow(None, 0, 64, 0)
    fake = C.c_void_p(8)   # a handle that is never followed: every refusal below comes in front of the scanner
    assert L.matchy_scanner_scan_gz_window(None, b"x", 1, C.byref(w), 1, False, C.byref(raw)) == INVALID and "gz_window" in M.last_error()
    assert L.matchy_scanner_scan_gz_window(fake, b"x", 1, C.byref(w), 1, False, None) == INVALID
    assert L.matchy_scanner_scan_gz_window(fake, b"x", 0, C.byref(w), 1, False, C.byref(raw)) == INVALID and "packed_len" in M.last_error()
    assert L.matchy_scanner_scan_gz_window(fake, None, 4, C.byref(w), 1, False, C.byref(raw)) == INVALID
    assert L.matchy_scanner_scan_gz_window(fake, b"x", 1, None, 1, False, C.byref(raw)) == INVALID and "window" in M.last_error()
    for bad, word in ((M._GzWindow(None, 65, 64, 0), "carry_cap"), (M._GzWindow(None, 3, 64, 0), "NULL"), (M._GzWindow(None, 0, 64, 2), "flag"),
                      (M._GzWindow(None, 0, 1 << 31, 0), "2^31")):
        assert L.matchy_scanner_scan_gz_window(fake, b"x", 1, C.byref(bad), 1, False, C.byref(raw)) == INVALID and word in M.last_error(), word
        assert L.matchy_multi_scanner_submit_gz_window(fake, b"x", 1, C.byref(bad), False, None) == INVALID and word in M.last_error(), word
    assert L.matchy_multi_scanner_submit_gz_window(None, b"x", 1, C.byref(w), False, None) == INVALID and "gz_window" in M.last_error()
    assert L.matchy_multi_scanner_submit_gz_window(fake, b"x", 0, C.byref(w), False, None) == INVALID
    assert L.matchy_scan_result_gz_window(None, None, None, None) == INVALID
    assert L.matchy_scan_result_gz_window(C.byref(raw), None, None, None) == INVALID and "window" in M.last_error()


def test_sources():
    hip = (ROOT / "matchy_amd" / "csrc" / "inflate.hip").read_text()
    for k in ("k_gz_inflate", "k_gz_seal", "k_gz_file_verdict", "k_gz_seal_files", "k_gz_window_tail"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    plan_h = (ROOT / "matchy_amd" / "csrc" / "gz_plan.h").read_text()
    assert "hip/" not in plan_h and plan_h.count("memmem(") == 1   # one copy of the cut rule
    import matchy_amd.build as B
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--gz-windows" in src and "matchy_multi_scanner_submit_gz_window" in src
