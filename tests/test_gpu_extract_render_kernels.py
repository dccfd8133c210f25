"""GPU: the kernels of csrc/extract_render.hip through their launch wrappers alone (csrc/extract_render.h), fed with candidate arrays,
against a sequential host model built from csrc/extract_render_core.h, at block capacities around and below the demand.

tests/hip/extract_render.hip holds the cases, the model and the comparison (read its head for what is asserted). It is compiled here,
from the test, with hipcc for gfx950 together with csrc/extract_render.hip, csrc/sort_hits.hip and csrc/line_index.hip into pytest's
temporary directory and run ONCE, as a child process with a time limit: one process, sequential launches. Every test below reads that
one run's report.

The contract these tests guard ("Extracted candidates as text"): the demand is counted past the capacity, nothing is stored at
or behind min(demand, capacity) or in front of the block, a block that fits is exact, padding entries are skipped, and both tiers of
candidates are exercised.
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

CASES = ["zero_entries", "padding_only", "one_candidate", "two_lists_padding", "n2047", "n2048", "n2049", "n4097", "eight_ranks_reverse",
         "newline_tile_edges", "no_newline", "ends_in_candidate", "escape_alignments", "long_candidates", "same_line_and_rank"]
RECORDS = {"zero_entries": 0, "padding_only": 0, "one_candidate": 1, "two_lists_padding": 300, "n2047": 2047, "n2048": 2048, "n2049": 2049,
           "n4097": 4097, "eight_ranks_reverse": 10, "newline_tile_edges": 4 * 3 + 5 + 1, "no_newline": 200, "ends_in_candidate": 2,
           "escape_alignments": 4 * sum(range(1, 10)), "long_candidates": 5, "same_line_and_rank": 300}
LINE = re.compile(r"^CASE (\S+) (.*?) (OK|FAIL: .*)$")


def constant(name):
    m = re.search(r"constexpr uint\d+_t %s = (\d+)" % name, (CSRC / "extract_render.h").read_text())
    return int(m.group(1))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("extract_render") / "extract_render"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", str(CSRC), str(ROOT / "tests" / "hip" / "extract_render.hip"),
                    str(CSRC / "extract_render.hip"), str(CSRC / "sort_hits.hip"), str(CSRC / "line_index.hip"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    rows = {}
    for line in r.stdout.splitlines():
        m = LINE.match(line)
        if m:
            fields = {k: int(v) for k, v in (kv.split("=") for kv in m.group(2).split())}
            rows.setdefault(m.group(1), []).append(dict(fields, verdict=m.group(3)))
    return r, rows


def test_harness_ran_to_its_end(report):
    r, rows = report
    done = re.search(r"^DONE cases=(\d+) failed=(\d+)$", r.stdout, re.M)
    assert done, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(done.group(1)) == sum(len(v) for v in rows.values())
    assert set(rows) == set(CASES)
    assert (r.returncode == 0) == (int(done.group(2)) == 0)


@pytest.mark.parametrize("case", CASES)
def test_block_against_the_host_model(report, case):
    r, rows = report
    mine = rows.get(case)
    assert mine, r.stdout[-2000:] + r.stderr[-2000:]
    for c in mine:
        print(case, c)
    bad = [c for c in mine if c["verdict"] != "OK"]
    assert not bad, bad
    assert {c["fmt"] for c in mine} == {0, 1, 2}
    for fmt in (0, 1, 2):
        runs = [c for c in mine if c["fmt"] == fmt]
        demand = {c["demand"] for c in runs}
        assert len(demand) == 1, demand   # counted past the capacity: the same at every capacity
        d = demand.pop()
        caps = [c["cap"] for c in runs]
        assert {c["records"] for c in runs} == {RECORDS[case]}
        if RECORDS[case] == 0:
            assert d == 0 and caps == [0, 1]
        else:
            assert d > 0 and caps == [0, d - 1, d, d + 1, 2 * d], (d, caps)
    # text is the shortest format, json the longest
    by_fmt = {c["fmt"]: c["demand"] for c in mine}
    assert by_fmt[2] <= by_fmt[1] <= by_fmt[0]


def test_both_tiers_and_the_tile_edges_ran(report):
    _, rows = report
    assert constant("XR_SHORT_MAX") == 512 and constant("XR_SCAN_CHUNK") == 2048 and constant("XR_KEY_TILE") == 2048
    longs = rows["long_candidates"][0]
    assert (longs["short"], longs["long"]) == (2, 3)   # 7 and 512 bytes stay with a lane; 513, 4099 and 100 000 go to a wave
    assert all(c["long"] == 0 for name in CASES if name != "long_candidates" for c in rows[name])
    assert rows["n4097"][0]["records"] > 2 * constant("XR_SCAN_CHUNK")   # the prefix sum and the sort run more than two workgroups
