"""CPU: the host side of hit lines — the C ABI surface (header, export list, library, ctypes mirror) and the constants the GPU tests
place their edge cases with."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

NEW_FUNCTIONS = ["matchy_scanner_set_hit_lines", "matchy_scanner_hit_lines", "matchy_scan_result_hit_lines", "matchy_scanner_get_hit_lines_timing",
                 "matchy_multi_scanner_set_hit_lines"]


def test_header_export_list_and_library_carry_the_hit_lines_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    assert ("typedef struct matchy_scan_hit_lines_t { const uint8_t *text; uint64_t text_len; uint32_t n_lines; "
            "const uint32_t *line_off, *line_no, *line_of_hit, *line_of_ip4_hit; } matchy_scan_hit_lines_t;") in flat
    assert re.search(r"int32_t matchy_scan_result_hit_lines\(const matchy_scan_result_t \*result, matchy_scan_hit_lines_t \*out\);", header)
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None


def test_ctypes_struct_has_the_layout_of_the_header():
    import matchy_amd as M
    names = [f[0] for f in M._ScanHitLines._fields_]
    assert names == ["text", "text_len", "n_lines", "line_off", "line_no", "line_of_hit", "line_of_ip4_hit"]
    S = M._ScanHitLines
    assert (S.text.offset, S.text_len.offset, S.n_lines.offset, S.line_off.offset, S.line_no.offset, S.line_of_hit.offset, S.line_of_ip4_hit.offset) == (0, 8, 16, 24, 32, 40, 48)
    assert C.sizeof(S) == 56


def test_exported_constants_are_the_kernels():
    import matchy_amd as M
    hh = (ROOT / "matchy_amd" / "csrc" / "hit_lines.h").read_text()
    assert int(re.search(r"HIT_LINES_SLICE = (\d+);", hh).group(1)) == M.HIT_LINES_SLICE
    assert int(re.search(r"HIT_LINES_SCAN_CHUNK = (\d+);", hh).group(1)) == M.HIT_LINES_SCAN_CHUNK
    assert M.HIT_LINES_SLICE % 16 == 0
    assert "hit_lines.hip" in (ROOT / "matchy_amd" / "build.py").read_text()


def test_null_handles_are_harmless_and_a_plain_result_is_refused():
    import matchy_amd as M
    L = M.lib()
    L.matchy_scanner_set_hit_lines(None, True)
    assert not L.matchy_scanner_hit_lines(None)
    L.matchy_multi_scanner_set_hit_lines(None, True)
    out = (C.c_float * 3)(7, 7, 7)
    L.matchy_scanner_get_hit_lines_timing(None, out)
    assert list(out) == [7, 7, 7]
    raw, h = M._ScanResult(), M._ScanHitLines()
    assert L.matchy_scan_result_hit_lines(None, C.byref(h)) != 0
    assert L.matchy_scan_result_hit_lines(C.byref(raw), None) != 0
    assert L.matchy_scan_result_hit_lines(C.byref(raw), C.byref(h)) != 0   # a result without the block
    assert "hit lines off" in M.last_error()
