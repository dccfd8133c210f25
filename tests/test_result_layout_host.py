"""CPU: the byte layout of the scanner's result blocks (csrc/result_layout.h: the pinned mirror and the block of the copy path), run
alone under AddressSanitizer + UBSan, and that the scanner computes it nowhere else."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"


def test_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "test_result_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(CSRC),
                    str(ROOT / "tests/cpp/test_result_layout.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "result layout: ok" in r.stdout


def test_the_offset_arithmetic_appears_once():
    """the padding of the id array to 8 bytes is result_layout.h's; engine.cpp only asks it"""
    pad = re.compile(r"\* 4\)? \+ 7\) & ~")
    assert len(pad.findall((CSRC / "result_layout.h").read_text())) == 1
    for name in ("engine.cpp", "engine.h"):
        assert not pad.search((CSRC / name).read_text()), name
    assert "result_layout.h" in (CSRC / "engine.h").read_text()
