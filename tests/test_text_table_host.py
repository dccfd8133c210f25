"""CPU: the device text table under the distinct-text set and the hit tally — its place in the build list and the layout logic the
host shares with the kernels (csrc/text_table.h: slot words, hash masking, pool words, table size, counter lines; csrc/lds_aggregator.h:
home slot and LDS size), run alone under AddressSanitizer + UBSan."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"


def test_sources_build_list_and_one_rehash_kernel():
    import matchy_amd.build as B
    assert "text_table.hip" in B.SOURCES
    assert re.search(r"__global__[^;{]*\bk_text_rehash\b", (CSRC / "text_table.hip").read_text())
    for name in ("distinct.hip", "tally.hip"):
        src = (CSRC / name).read_text()
        assert "text_table.h" in (CSRC / name.replace(".hip", ".h")).read_text()
        assert not re.search(r"__global__[^;{]*rehash", src), name


def test_layout_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "test_text_table_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", str(CSRC), str(ROOT / "tests/cpp/test_text_table_layout.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "text table layout: ok" in r.stdout
