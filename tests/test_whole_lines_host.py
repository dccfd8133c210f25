"""CPU: the host side of whole-line queries — the C ABI surface (header, export list, library, Python mirror), the two answerers of the
model held against each other on the case inputs, and csrc/whole_lines_core.h built into a stand-alone program under AddressSanitizer +
UBSan and compared with the Python model of tests/whole_lines_cases.py (line cuts, the '\\r' rule, UTF-8 verdicts, classification)."""
import ctypes as C
import ipaddress
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whole_lines_cases as W   # noqa: E402

ROOT = W.ROOT

NEW_FUNCTIONS = ["matchy_scanner_set_whole_lines", "matchy_scanner_whole_lines", "matchy_scanner_get_whole_lines_counters",
                 "matchy_scanner_get_whole_lines_timing", "matchy_multi_scanner_set_whole_lines"]


def test_header_export_list_library_and_mirror_carry_the_whole_line_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"void\s+matchy_scanner_set_whole_lines\s*\(\s*matchy_scanner_t\s*\*\s*\w+,\s*bool\s+\w+\)", header)
    assert re.search(r"bool\s+matchy_scanner_whole_lines\s*\(\s*const\s+matchy_scanner_t\s*\*\s*\w+\)", header)
    assert re.search(r"void\s+matchy_scanner_get_whole_lines_counters\s*\(\s*const\s+matchy_scanner_t\s*\*\s*\w+,\s*uint64_t\s+\w+\[4\]\)", header)
    assert re.search(r"void\s+matchy_scanner_get_whole_lines_timing\s*\(\s*const\s+matchy_scanner_t\s*\*\s*\w+,\s*float\s+\w+\[3\]\)", header)
    assert re.search(r"int32_t\s+matchy_multi_scanner_set_whole_lines\s*\(\s*matchy_multi_scanner_t\s*\*\s*\w+,\s*bool\s+\w+\)", header)
    # null handles are refused or ignored, not dereferenced
    INVALID = -5
    L.matchy_scanner_set_whole_lines(None, True)
    assert L.matchy_scanner_whole_lines(None) is False
    ctr = (C.c_uint64 * 4)(7, 7, 7, 7)
    L.matchy_scanner_get_whole_lines_counters(None, ctr)
    assert list(ctr) == [7, 7, 7, 7]
    ms = (C.c_float * 3)(1, 1, 1)
    L.matchy_scanner_get_whole_lines_timing(None, ms)
    assert list(ms) == [1, 1, 1]
    assert L.matchy_multi_scanner_set_whole_lines(None, True) == INVALID
    for cls, attrs in ((M.Scanner, ("set_whole_lines", "whole_lines_enabled", "whole_lines_counters", "whole_lines_timing_ms")), (M.MultiScanner, ("set_whole_lines",))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)


def test_sources_build_list_and_command_line():
    import matchy_amd.build as B
    assert "whole_lines.hip" in B.SOURCES
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--whole-lines" in src and "matchy_multi_scanner_set_whole_lines" in src
    hip = (ROOT / "matchy_amd" / "csrc" / "whole_lines.hip").read_text()
    for k in ("k_wl_scatter", "k_wl_classify"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    core = (ROOT / "matchy_amd" / "csrc" / "whole_lines_core.h").read_text()
    assert "hip/" not in core
    W.expected_sizes_ok()


def test_python_line_split():
    assert W.split_lines(b"") == []
    assert W.split_lines(b"\n") == [(0, 0)]
    assert W.split_lines(b"a") == [(0, 1)]
    assert W.split_lines(b"a\n") == [(0, 1)]
    assert W.split_lines(b"\n\n\n") == [(0, 0), (1, 1), (2, 2)]
    assert W.split_lines(b"a\r\nb\r\r\n\rc") == [(0, 1), (3, 5), (7, 9)]
    assert W.split_lines(b"\r") == [(0, 0)]


def all_case_buffers():
    u = W.kernel_units()
    out = {"rules": W.rule_list(), "repeats": W.repeats_list()}
    for i, bad in enumerate(W.BAD_SEQUENCES):
        out["invalid%d" % i] = W.invalid_list(bad)
    for unit in (u["WL_LANE_BYTES"], u["WL_TILE"]):
        for name, buf in W.boundary_lists(unit, 3 * unit).items():
            out["%s@%d" % (name, 3 * unit)] = buf
    for k, b in enumerate((b"", b"\n", b"a", b"a\n", b"\n\n\n", b"\n" * 70 + b"evil.com\n", b"evil.com\n10.1.2.3")):
        out["cut%d" % k] = b
    return out


@pytest.mark.parametrize("ci", [False, True])
def test_the_two_answerers_agree_on_every_case_line(oracle, ci, tmp_path):
    """oracle.Database.lookup and the library's host path (csrc/host_lookup.cpp, built alone under ASan / UBSan: a handle of the
    library is not opened without a GPU) give the same answer wherever both apply, and the embedded-IPv4 lines give what is written
    out by hand (the assertions are in W.model)"""
    from test_host_units import _host_answers, _host_lookup_exe
    exe = _host_lookup_exe(tmp_path)
    u = W.kernel_units()
    buffers = [W.rule_list(), W.repeats_list()] + [W.invalid_list(bad) for bad in W.BAD_SEQUENCES]
    buffers += list(W.boundary_lists(u["WL_TILE"], u["WL_TILE"]).values())
    blob = W.build_blob(W.rule_entries(), case_insensitive=ci)
    queries = sorted({q for buf in buffers for q in W.valid_queries(buf)})
    answers = dict(zip(queries, _host_answers(exe, blob, [q.decode("utf-8") for q in queries], tmp_path)))
    host = W.host_from_cli(answers)
    odb = oracle.Database(blob)
    try:
        recs, ctr = W.model(odb, host, W.rule_list())
        by_query = {W.rule_list()[r["start"]:r["end"]]: r for r in recs}
        # a few answers by eye, so that a model that finds nothing does not pass
        assert by_query[b"192.0.2.7"]["prefix_len"] == 32 and by_query[b"10.1.2.99"]["prefix_len"] == 24
        assert by_query[b"fe80::1"]["kind"] == "ip" and by_query[b"1.2.3"]["kind"] == "pattern"
        assert by_query[b"::ffff:192.0.2.1"]["prefix_len"] == 120 and by_query[b"::ffff:192.0.2.1"]["data"] == [{"k": "mapped"}]
        assert len(by_query[b"both.evil.org"]["ids"]) == 4
        assert (b"EXAMPLE.COM" in by_query) == ci
        for miss in (b"01.2.3.4", b"1.2.3.4/32", b" 1.2.3.4", b"1.2.3.4 ", b"fe80::1%eth0", b"foo.com", W.HEX47, b"good.com", b""):
            assert miss not in by_query, miss
        assert b"foo.com." in by_query and b"evil.com" in by_query and b"hello wide world" in by_query
        assert ctr["queries"] == len(W.RULE_QUERIES) + 1 and ctr["invalid_utf8"] == 0
        assert ctr["address"] == sum(W.classify(q) != "str" for q in W.RULE_QUERIES) + 1
        for buf in buffers[1:]:
            W.model(odb, host, buf)
        for bad in W.BAD_SEQUENCES:
            buf = W.invalid_list(bad)
            recs, ctr = W.model(odb, host, buf)
            assert ctr["invalid_utf8"] == 3 and ctr["queries"] == 7, (bad, ctr)
            assert [buf[r["start"]:r["end"]] for r in recs] == [b"evil.com", b"192.0.2.7", "\u20acevil".encode(), b"evil.com"], bad
    finally:
        odb.close()


# ------------------------------------------------------------------------------------------------ the rules header
@pytest.fixture(scope="module")
def core(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wl_core") / "test_whole_lines_core"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "cpp" / "test_whole_lines_core.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def run_core(exe, tmp_path, buf):
    path = tmp_path / "buf.bin"
    path.write_bytes(buf)
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines, total = [], None
    for row in p.stdout.splitlines():
        w = row.split()
        if w[0] == "L":
            lines.append((int(w[2]), int(w[3]), int(w[4]), int(w[5]), w[6]))
        else:
            total = (int(w[1]), int(w[2]))
    return lines, total


def python_rows(buf):
    rows = []
    for s, e in W.split_lines(buf):
        q = buf[s:e]
        cls = W.classify(q)
        addr = "-"
        if cls == "ip4":
            addr = ipaddress.IPv4Address(q.decode()).packed.hex()
        elif cls == "ip6":
            addr = ipaddress.IPv6Address(q.decode()).packed.hex()
        # the verdict on UTF-8 is the line's ('\r' included: it is ASCII and changes nothing)
        rows.append((s, e, {"str": 0, "ip4": 1, "ip6": 2}[cls], 0 if W.utf8_ok(q) else 1, addr))
    return rows


def test_core_header_against_the_python_model_on_every_case_input(core, tmp_path):
    for name, buf in all_case_buffers().items():
        got, total = run_core(core, tmp_path, buf)
        want = python_rows(buf)
        assert got == want, name
        assert total == (len(want), buf.count(b"\n")), name


def test_core_header_utf8_verdict_per_byte_matches_python_on_all_short_sequences(core, tmp_path):
    """every sequence of up to three bytes from a set that holds each class of byte (ASCII, '\\n', continuation bytes at the range
    limits, leads of every length, the leads with a narrowed second byte, bytes that begin nothing), one per line, and a four-byte
    sweep around the limits — the per-byte rule must give the line the verdict bytes.decode gives it"""
    alphabet = [0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF]
    seqs = [bytes([a]) for a in alphabet] + [bytes([a, b]) for a in alphabet for b in alphabet]
    seqs += [bytes([a, b, c]) for a in alphabet for b in alphabet for c in (0x41, 0x80, 0x9F, 0xA0, 0xBF, 0xC2, 0xF0)]
    seqs += [bytes([a, b, 0x80, c]) for a in (0xF0, 0xF1, 0xF4, 0xE0, 0xED) for b in (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0) for c in (0x41, 0x80, 0xBF, 0xC0)]
    buf = b"\n".join(seqs)   # the last one ends the buffer
    got, total = run_core(core, tmp_path, buf)
    want = python_rows(buf)
    assert len(got) == len(want) == len(seqs)
    bad = [(seqs[i], got[i], want[i]) for i in range(len(seqs)) if got[i] != want[i]]
    assert not bad, bad[:5]


def test_core_header_address_texts(core, tmp_path):
    qs = [b"0.0.0.0", b"255.255.255.255", b"256.1.1.1", b"1.2.3.4.5", b"1..2.3", b"1.2.3.04", b"0x1.2.3.4", b"::", b"::1", b"1::", b":::", b"1:2:3:4:5:6:7:8",
          b"1:2:3:4:5:6:7:8:9", b"1:2:3:4:5:6:7::", b"::2:3:4:5:6:7:8", b"1::8::9", b"12345::", b"g::1", b"::ffff:1.2.3.4", b"::1.2.3", b"1.2.3.4::",
          b"1:2:3:4:5:6:1.2.3.4", b"1:2:3:4:5:6:7:1.2.3.4", b"ffff:ffff:ffff:ffff:ffff:ffff:255.255.255.255", b"ffff:ffff:ffff:ffff:ffff:ffff:255.255.255.2555",
          b"[::1]", b"::1%lo", b"::1/128", b" ::1", b"::1 ", b"FE80::ABCD", b"1:2:3:4:5:6:7:8\r", b"-1.2.3.4", b"+1.2.3.4", b"1.2.3.4\x00"]
    buf = b"\n".join(qs) + b"\n"
    got, total = run_core(core, tmp_path, buf)
    assert got == python_rows(buf)
    assert total == (len(qs), len(qs))
