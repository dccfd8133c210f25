"""CPU: the host side of the distinct-text set — the C ABI surface (header, export list, library) and the layout logic the host shares
with the kernels (csrc/distinct.h: order key, slot states; the table's own layout is in test_text_table_host.py), run alone under
AddressSanitizer + UBSan."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

NEW_FUNCTIONS = ["matchy_amd_extractor_set_unique", "matchy_amd_extractor_unique", "matchy_amd_extractor_reset_unique",
                 "matchy_amd_extractor_unique_count"]


def test_header_export_list_and_library_carry_the_unique_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"uint64_t\s+matchy_amd_extractor_unique_count\s*\(\s*const matchy_extractor_t", header)
    assert re.search(r"void\s+matchy_amd_extractor_set_unique\s*\(\s*matchy_extractor_t\s*\*\s*\w+,\s*bool", header)
    # a null handle is harmless and reports "off" / nothing seen
    L.matchy_amd_extractor_set_unique(None, True)
    L.matchy_amd_extractor_reset_unique(None)
    assert not L.matchy_amd_extractor_unique(None) and L.matchy_amd_extractor_unique_count(None) == 0
    # the Python mirror
    for attr in ("set_unique", "reset_unique", "unique_count", "unique"):
        assert hasattr(M.Extractor, attr), attr


def test_command_line_keeps_no_host_set():
    import matchy_amd.build as B
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "seen_sorted" not in src and "seen_new" not in src
    assert "matchy_amd_extractor_set_unique" in src


def test_layout_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "test_distinct_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests/cpp/test_distinct_layout.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "distinct layout: ok" in r.stdout
