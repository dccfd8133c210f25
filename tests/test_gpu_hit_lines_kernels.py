"""GPU: the kernels of csrc/hit_lines.hip through their launch wrappers alone (csrc/hit_lines.h), against a sequential host model, at
block capacities around and below the demand.

tests/hip/hit_lines.hip holds the cases, the model and the comparison (read its head for what is asserted). It is compiled here, from
the test, with hipcc for gfx950 together with csrc/hit_lines.hip into pytest's temporary directory and run ONCE, as a child process
with a time limit: one process, sequential launches. Every test below reads that one run's report.

The contract these tests guard ("Hit lines"): the demand is counted past the capacity, nothing is stored at or behind
min(demand, capacity) or in front of the block, and a block that fits is exact. A copy kernel that breaks it is invisible to the
whole-scan tests once the scanner's block has grown.
"""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CASES = (["residues", "slice_edge-1", "slice_edge+0", "slice_edge+1", "long_line", "many_lines", "empty"]
         + ["unterminated%d" % t for t in (1, 15, 16, 17, 100, 5000)])
CASE = re.compile(r"^CASE (\S+) cap=(\d+) demand=(\d+) lines=(\d+) records=(\d+) (OK|FAIL: .*)$")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hit_lines") / "hit_lines"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", str(CSRC), str(ROOT / "tests" / "hip" / "hit_lines.hip"),
                    str(CSRC / "hit_lines.hip"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    cases = {}
    for line in r.stdout.splitlines():
        m = CASE.match(line)
        if m:
            cases.setdefault(m.group(1), []).append(dict(cap=int(m.group(2)), demand=int(m.group(3)), lines=int(m.group(4)), records=int(m.group(5)),
                                                         verdict=m.group(6)))
    return r, cases


def test_harness_ran_to_its_end(report):
    r, cases = report
    done = re.search(r"^DONE cases=(\d+) failed=(\d+)$", r.stdout, re.M)
    assert done, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(done.group(1)) == sum(len(v) for v in cases.values())
    assert set(cases) == set(CASES), sorted(set(cases) ^ set(CASES))
    assert (r.returncode == 0) == (int(done.group(2)) == 0)


@pytest.mark.parametrize("case", CASES)
def test_block_against_the_host_model(report, case):
    r, cases = report
    mine = cases.get(case)
    assert mine, r.stdout[-2000:] + r.stderr[-2000:]
    for c in mine:
        print(case, c)
    bad = [c for c in mine if c["verdict"] != "OK"]
    assert not bad, bad
    demand = {c["demand"] for c in mine}
    assert len(demand) == 1, demand   # counted past the capacity: the same at every capacity
    d = demand.pop()
    caps = [c["cap"] for c in mine]
    if case == "empty":
        assert d == 0 and mine[0]["lines"] == 0 and caps == [0, 1]
    else:
        assert d > 0 and caps == [0, d - 1, d, d + 1, 2 * d], (d, caps)


def test_shapes_of_the_cases(report):
    import matchy_amd as M
    _, cases = report
    S = M.HIT_LINES_SLICE
    assert cases["residues"][0]["lines"] == 1 + 16 * 41 and cases["residues"][0]["records"] == 1 + 16 * 41 + 199
    assert cases["long_line"][0]["demand"] == 13 + 3 * S + 6 + 13
    assert cases["many_lines"][0]["lines"] > M.HIT_LINES_SCAN_CHUNK   # the offset step runs more than one workgroup
    for d, name in ((-1, "slice_edge-1"), (0, "slice_edge+0"), (1, "slice_edge+1")):
        assert cases[name][0]["demand"] == (S + d) + 200 * 21 + (2 * S - 6001 - d + 1) + 34
