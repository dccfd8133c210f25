"""CPU: the bit-sliced label rules of k_validate_dom (matchy_amd/csrc/domain_planes.h), compiled with g++: the class masks of a context
record for every byte value at every position, and the rule function against the SWAR function it replaced and against a byte loop,
on constructed and random contexts. No GPU."""
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_context_planes_and_domain_rules(tmp_path):
    """context_planes(): 256 byte values x 32 positions (on six backgrounds), every bit of DC, DOT, DASH, HIGH and B equals the class of its
    byte. domain_rules(): verdict, start and end equal those of both references on every combination of the seven byte classes on the six
    bytes in front of the label, every run length 0..24 with j == 24 and j > 24, every label length 1..8 with every class of stop byte,
    labels that alone are a suffix and labels that are not, min_labels 1..3, and 12 M random contexts; every verdict occurs at least
    1000 times."""
    exe = tmp_path / "test_domain_planes"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests/cpp/test_domain_planes.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "domain_planes ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert re.search(r"^context_planes: 0 wrong bits", r.stdout, re.M), r.stdout[-4000:]
    assert re.search(r"^mismatches 0$", r.stdout, re.M), r.stdout[-4000:]
    m = re.search(r"^cases (\d+) \(constructed (\d+), random (\d+)\)", r.stdout, re.M)
    assert m and int(m.group(3)) >= 10_000_000, r.stdout[-4000:]
    m = re.search(r"^verdicts: 0 (\d+)  1 (\d+)  2 (\d+)", r.stdout, re.M)
    assert m, r.stdout[-4000:]
    for verdict, n in enumerate(map(int, m.groups())):
        assert n >= 1000, (verdict, n)
