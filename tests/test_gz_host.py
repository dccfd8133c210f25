"""CPU: the host side of gz scans — the C ABI surface (header, export list, library, Python mirror), the status constants, and the calls'
parameter checks, which refuse NULL handles and bad tables without a dereference. No GPU."""
import ctypes as C
import re
from pathlib import Path

import gz_cases as G

ROOT = Path(__file__).resolve().parent.parent

NEW_FUNCTIONS = {"matchy_scanner_scan_gz": "int32_t", "matchy_scan_result_gz": "int32_t", "matchy_multi_scanner_submit_gz": "int32_t",
                 "matchy_scanner_get_gz_timing": "void"}
INVALID = -5


def test_header_export_list_library_and_mirror_carry_the_gz_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name, ret in NEW_FUNCTIONS.items():
        assert re.search(r"%s\s+%s\s*\(" % (ret, name), header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"typedef struct matchy_gz_member_t \{ uint64_t offset; uint32_t len; uint32_t out_len; \} matchy_gz_member_t;", header)
    assert C.sizeof(M._GzMember) == 16 and M._GzMember.len.offset == 8 and M._GzMember.out_len.offset == 12
    assert re.search(r"matchy_scanner_scan_gz\s*\(\s*matchy_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const matchy_gz_member_t\s*\*\s*\w+,"
                     r"\s*size_t\s+\w+,\s*uint32_t\s+\w+,\s*bool\s+\w+,\s*matchy_scan_result_t\s*\*\s*\w+\)", header)
    assert re.search(r"matchy_multi_scanner_submit_gz\s*\(\s*matchy_multi_scanner_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*size_t\s+\w+,\s*const matchy_gz_member_t\s*\*\s*\w+,"
                     r"\s*size_t\s+\w+,\s*bool\s+\w+,\s*void\s*\*\s*\w+\)", header)
    for cls, attrs in ((M.Scanner, ("scan_gz", "gz_timing_ms")), (M.MultiScanner, ("submit_gz_ptr",)), (M.ScanResult, ("gz_status", "gz_text", "gz_text_len"))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)


def test_status_constants_agree():
    """header, Python mirror, the vectors' names and the decoder's enum carry the same eleven values"""
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    core = (ROOT / "matchy_amd" / "csrc" / "inflate_core.h").read_text()
    assert M.GZ_STATUS_NAMES == G.STATUS and len(G.STATUS) == 11
    for value, name in enumerate(G.STATUS):
        assert re.search(r"#define MATCHY_GZ_%s %d\b" % (name, value), header), name
        assert getattr(M, "GZ_" + name) == value
        assert re.search(r"\bGZ_%s = %d\b" % (name, value), core), name


def test_null_handles_and_bad_tables_are_refused():
    import matchy_amd as M
    L = M.lib()
    raw = M._ScanResult()
    table = (M._GzMember * 1)()
    assert L.matchy_scanner_scan_gz(None, None, 0, None, 0, 1, False, None) == INVALID
    assert L.matchy_scanner_scan_gz(None, b"x", 1, table, 1, 1, False, C.byref(raw)) == INVALID
    assert L.matchy_scan_result_gz(None, None, None, None, None) == INVALID
    assert L.matchy_scan_result_gz(C.byref(raw), None, None, None, None) == INVALID and "gz scan" in M.last_error()
    assert L.matchy_multi_scanner_submit_gz(None, None, 0, None, 0, False, None) == INVALID
    out = (C.c_float * 3)(7, 7, 7)
    L.matchy_scanner_get_gz_timing(None, out)   # harmless
    assert list(out) == [7, 7, 7]


def test_sources_and_build_list():
    import matchy_amd.build as B
    assert "inflate.hip" in B.SOURCES
    hip = (ROOT / "matchy_amd" / "csrc" / "inflate.hip").read_text()
    for k in ("k_gz_inflate", "k_gz_seal"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--gz-on-gpu" in src and "matchy_multi_scanner_submit_gz" in src and "MATCHY_AMD_GZ_MAX_MEMBER" in src
    for host_only in ("gz_plan.h",):
        assert "hip/" not in (ROOT / "matchy_amd" / "csrc" / host_only).read_text()


def test_layout_model():
    """the model the GPU tests lay their expected batches out with, on members small enough to check by eye"""
    starts, buf = G.layout([(3, b"abc"), (0, b""), (2, None), (2, b"x\n"), (0, None)])
    assert starts == [0, 4, 4, 7, 10] and buf == b"abc\n" + b"\n\n\n" + b"x\n\n"
