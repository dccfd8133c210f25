"""CPU: the host side of segmented scans — the C ABI surface (header, export list, library, Python mirror), and the input packer of
`matchy match --pack-inputs` (csrc/input_packer.h) built alone under AddressSanitizer + UBSan and compared with a Python model."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import segment_cases as S   # noqa: E402

ROOT = S.ROOT

NEW_FUNCTIONS = ["matchy_scanner_set_segments", "matchy_scan_result_segments", "matchy_scan_result_to_ndjson_segments",
                 "matchy_multi_scanner_submit_segments"]
STRUCT = """typedef struct matchy_scan_segment_t {
  uint32_t start, len;
  uint32_t hits;
  uint32_t line_base;
  uint32_t lines;
  uint32_t lines_with_matches;
  uint32_t reserved[2];
} matchy_scan_segment_t;"""


def test_header_export_list_library_and_mirror_carry_the_segment_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS + ["matchy_scan_segment_t"]:
        assert re.search(r"\b%s\b" % name, header), name
    for name in NEW_FUNCTIONS:
        assert re.search(r"int32_t\s+%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    # the struct text, comments aside
    plain = re.sub(r"[ \t]*/\*.*?\*/", "", header, flags=re.S)
    plain = "\n".join(line.rstrip() for line in plain.splitlines())
    assert STRUCT in plain
    assert re.search(r"matchy_scanner_set_segments\s*\(\s*matchy_scanner_t\s*\*\s*\w+,\s*const uint32_t\s*\*\s*\w+,\s*size_t\s+\w+\)", header)
    assert re.search(r"matchy_multi_scanner_submit_segments\s*\(\s*matchy_multi_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const uint32_t\s*\*\s*\w+,\s*size_t\s+\w+,"
                     r"\s*void\s*\*\s*\w+,\s*const void\s*\*\s*\w+\)", header)
    assert C.sizeof(M._ScanSegment) == 32 and M._ScanSegment.lines_with_matches.offset == 20
    # null handles are refused, not dereferenced
    INVALID = -5
    assert L.matchy_scanner_set_segments(None, None, 0) == INVALID
    assert L.matchy_scan_result_segments(None, None, None, None, None) == INVALID
    assert L.matchy_multi_scanner_submit_segments(None, None, 0, None, 0, None, None) == INVALID
    out, n = C.c_void_p(), C.c_size_t()
    assert L.matchy_scan_result_to_ndjson_segments(None, None, None, None, None, False, C.byref(out), C.byref(n)) == INVALID
    raw = M._ScanResult()
    assert L.matchy_scan_result_segments(C.byref(raw), None, None, None, None) == INVALID and "without segments" in M.last_error()
    for cls, attrs in ((M.Scanner, ("set_segments",)), (M.MultiScanner, ("submit_segments_ptr",)), (M.ScanResult, ("segments", "segment_of", "segment_of_ip4", "ndjson_segments_text"))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)


def test_sources_build_list_and_command_line():
    import matchy_amd.build as B
    assert "segments.hip" in B.SOURCES
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--pack-inputs" in src and "matchy_multi_scanner_submit_segments" in src and "matchy_scan_result_to_ndjson_segments" in src
    hip = (ROOT / "matchy_amd" / "csrc" / "segments.hip").read_text()
    for k in ("k_seg_build", "k_seg_records", "k_seg_lines"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    packer = (ROOT / "matchy_amd" / "csrc" / "input_packer.h").read_text()
    assert "hip/" not in packer


def test_host_model_of_the_segment_passes():
    """the model the GPU tests compare with, on a buffer small enough to check by eye"""
    buf, starts = S.pack([b"", b"a\nb\n", b"", b"\n", b"c"])
    assert starts == [0, 0, 4, 4, 5]
    hits = [0, 2, 5]
    assert list(S.segment_of(starts, hits)) == [1, 1, 4]
    assert S.table_model(buf, starts, hits, True) == [(0, 0, 0, 0, 0, 0), (0, 4, 2, 0, 2, 2), (4, 0, 0, 2, 0, 0), (4, 1, 0, 2, 1, 0), (5, 1, 1, 3, 0, 1)]
    assert S.table_model(buf, starts, hits, False) == [(0, 0, 0, 0, 0, 0), (0, 4, 2, 0, 0, 0), (4, 0, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0), (5, 1, 1, 0, 0, 0)]


# ------------------------------------------------------------------------------------------------ the packer
@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = tmp_path_factory.mktemp("packer") / "test_input_packer"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           str(ROOT / "tests" / "cpp" / "test_input_packer.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def run_packer(exe, batch_bytes, paths):
    p = subprocess.run([str(exe), str(batch_bytes)] + [str(x) for x in paths], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    plan, stats = [], None
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "pack":
            plan.append(("pack", [tuple(int(x) for x in e.split(":")) for e in w[2:]], bytes.fromhex(w[1])))
        elif w[0] == "stats":
            stats = (int(w[1]), int(w[2]))
        else:
            plan.append((w[0], int(w[1])))
    return plan, stats


def write_files(d, files):
    """files: [(name, bytes or None, kind)]; returns the paths and the model's input"""
    paths, model = [], []
    for name, data, kind in files:
        path = d / name
        if kind == "missing":
            model.append((b"", "ineligible"))
        elif kind == "dir":
            path.mkdir()
            model.append((b"", "ineligible"))
        else:
            path.write_bytes(data)
            if kind == "unreadable":
                path.chmod(0)
                kind = "ok" if os.access(path, os.R_OK) else "unreadable"   # a privileged user reads it anyway
            model.append((data, "ineligible" if name.endswith(".gz") else kind))
        paths.append(path)
    return paths, model


def check_plan(exe, d, files, batch_bytes):
    paths, model = write_files(d, files)
    want = S.pack_model(model, batch_bytes)
    got, stats = run_packer(exe, batch_bytes, paths)
    assert got == want
    packs = [p for p in want if p[0] == "pack"]
    assert stats == (sum(len(p[1]) for p in packs), len(packs))
    return want


def test_packer_final_newlines_crlf_and_empty_files(packer, tmp_path):
    files = [("a.log", b"one\ntwo\n", "ok"), ("b.log", b"no final newline", "ok"), ("c.log", b"crlf line\r\nsecond\r\n", "ok"), ("d.log", b"crlf open\r", "ok"),
             ("e.log", b"\n", "ok"), ("f.log", b"x", "ok")]
    want = check_plan(packer, tmp_path, files, 4096)
    assert want == [("pack", [(0, 0, 0), (1, 8, 1), (2, 25, 0), (3, 44, 1), (4, 55, 0), (5, 56, 1)],
                     b"one\ntwo\nno final newline\ncrlf line\r\nsecond\r\ncrlf open\r\n\nx\n")]
    d2 = tmp_path / "empties"
    d2.mkdir()
    files = [("a.log", b"first\n", "ok"), ("empty1", b"", "ok"), ("b.log", b"second\n", "ok"), ("c.log", b"third\n", "ok"), ("empty2", b"", "ok")]
    want = check_plan(packer, d2, files, 4096)
    assert want == [("single", 0), ("single", 1), ("pack", [(2, 0, 0), (3, 7, 0)], b"second\nthird\n"), ("single", 4)]   # an empty file is read the old way


def test_packer_room_limit_and_order(packer, tmp_path):
    B = 4096
    # seven files leave 24 bytes of room: a file of exactly that (with its final newline, or one byte shorter and in need of one) joins
    # the pack; one byte more (24 bytes without a final newline, 25 with) opens the next pack together with the file behind it
    for k, (size, nl, same_pack) in enumerate([(24, True, True), (23, False, True), (24, False, False), (25, True, False)]):
        d = tmp_path / f"room{k}"
        d.mkdir()
        last = b"z" * (size - 1) + (b"\n" if nl else b"z")
        files = [(f"s{j}.log", b"x" * 249 + b"\n", "ok") for j in range(4)] + [(f"m{j}.log", b"y" * 1023 + b"\n", "ok") for j in range(3)]
        files += [("last.log", last, "ok"), ("after.log", b"tail\n", "ok")]
        want = check_plan(packer, d, files, B)
        first = want[0]
        assert first[0] == "pack" and len(first[1]) == (8 if same_pack else 7), (k, want)
        assert len(first[2]) == (B if same_pack else B - 24), k
        assert want[1:] == ([("single", 8)] if same_pack else [("pack", [(7, 0, 0 if nl else 1), (8, size + (0 if nl else 1), 0)], last + (b"" if nl else b"\n") + b"tail\n")]), k
    # a file above the limit between two small ones, twice: order kept, the lone small files go the old way, the pairs are packs
    d = tmp_path / "order"
    d.mkdir()
    files = [("a.log", b"a\n", "ok"), ("b.log", b"b\n", "ok"), ("big.log", b"B" * (B // 4 + 1), "ok"), ("c.log", b"c\n", "ok"), ("d.log", b"d", "ok"),
             ("at_limit.log", b"L" * (B // 4), "ok"), ("e.log", b"e\n", "ok")]
    want = check_plan(packer, d, files, B)
    assert [w[0] for w in want] == ["pack", "single", "pack"] and want[1] == ("single", 2)
    assert [e[0] for e in want[0][1]] == [0, 1] and [e[0] for e in want[2][1]] == [3, 4, 5, 6]


def test_packer_inputs_it_must_not_pack(packer, tmp_path):
    files = [("a.log", b"a\n", "ok"), ("gone.log", None, "missing"), ("b.log", b"b\n", "ok"), ("c.log", b"c\n", "ok"), ("z.log.gz", b"\x1f\x8b not really", "ok"),
             ("d.log", b"d\n", "ok"), ("locked.log", b"secret\n", "unreadable"), ("e.log", b"e\n", "ok"), ("sub", None, "dir"), ("f.log", b"f\n", "ok")]
    want = check_plan(packer, tmp_path, files, 4096)
    assert want[:4] == [("single", 0), ("single", 1), ("pack", [(2, 0, 0), (3, 2, 0)], b"b\nc\n"), ("single", 4)]
    assert want[-2:] == [("single", 8), ("single", 9)]
    # an eligible file that cannot be opened, whoever runs the test: the first pack that goes out takes the last file descriptor the
    # process allows itself. The files behind it are reported and the walk goes on: nothing is packed from then on, order is kept
    d = tmp_path / "starved"
    d.mkdir()
    B = 4096
    files = [("a.log", b"a\n", "ok"), ("b.log", b"b", "ok"), ("big.log", b"B" * (B // 4 + 1), "ok"), ("c.log", b"c\n", "unreadable"), ("d.log", b"d\n", "unreadable"),
             ("sub", None, "dir"), ("e.log", b"e" * 1000 + b"\n", "unreadable"), ("f.log", b"f" * 1000 + b"\n", "unreadable"), ("g.log", b"g" * 1000 + b"\n", "unreadable"),
             ("h.log", b"h" * 1000 + b"\n", "unreadable"), ("i.log", b"i" * 1000 + b"\n", "unreadable")]
    paths, model = [], []
    for name, data, kind in files:
        if kind == "dir":
            (d / name).mkdir()
            model.append((b"", "ineligible"))
        else:
            (d / name).write_bytes(data)
            model.append((data, kind))
        paths.append(d / name)
    want = S.pack_model(model, B)
    got, stats = run_packer(packer, "!%d" % B, paths)
    assert got == want == [("pack", [(0, 0, 0), (1, 2, 1)], b"a\nb\n"), ("single", 2), ("error", 3), ("error", 4), ("single", 5)] + [("error", k) for k in range(6, 11)]
    assert stats == (2, 1)
    # a single eligible file goes the old way; so does "-"
    d = tmp_path / "one"
    d.mkdir()
    assert check_plan(packer, d, [("only.log", b"only\n", "ok")], 4096) == [("single", 0)]
    got, stats = run_packer(packer, 4096, ["-", d / "only.log"])
    assert got == [("single", 0), ("single", 1)] and stats == (0, 0)
