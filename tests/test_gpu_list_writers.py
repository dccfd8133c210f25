"""GPU: the wave-level list writers (ChunkWriter, BufferedWriter, StagedChunkWriter, DomWriter in csrc/device_common.h) against a
sequential host model, at capacities around and below their demand.

tests/hip/list_writers.hip holds one small kernel per writer, the model and the comparison (read its head for what is asserted). It is
compiled here, from the test, with hipcc for gfx950 into pytest's temporary directory and run ONCE, as a child process with a time limit:
one process, sequential launches, bounded loops. Every test below reads that one run's report.

The list contract these tests guard ("The work lists"): count past the capacity, never write past it, pad what you reserve.
A writer that breaks it is still invisible to the whole-scan tests: the regrow-and-rescan path repairs the result.

SparseWriter / LaneHeldWriter (k_anchor.hip) are NOT in the harness. They fetch their destination from k_anchor's kernel-argument
segment (cold_tok()), so lifting them means a template parameter or a header for the writer and a check that k_anchor's gfx950
assembly stays identical; that move was not attempted here. They are covered only indirectly, by the `rare` and `tok` lists of
tests/test_gpu_overflow.py at whatever tok_chunk / rare_chunk hint the previous scan left (0 on the first scan of a scanner); the
hints 64 and 4032 are not driven on purpose by any test.
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

# every instantiation the kernels use (lookup_kernels.hip, validate_kernels.hip, k_anchor.hip)
WRITERS = [
    "ChunkWriter<Hit,HIT_CHUNK>",
    "ChunkWriter<Candidate,CAND_CHUNK>",
    "BufferedWriter<Candidate>",
    "BufferedWriter<RareAnchor>",
    "BufferedWriter<uint32_t>",
    "BufferedWriter<uint2,RARE_STAGE>",
    "StagedChunkWriter<Candidate,CAND_STAGE>/64",
    "StagedChunkWriter<Candidate,CAND_STAGE>/1024",
    "DomWriter/static/256",
    "DomWriter/static/1024",
    "DomWriter/reserved/256",
    "DomWriter/reserved/1024",
]
WAVES = (1, 4, 320)
# reservation sizes a capacity must have cut through in at least one case of the writer (the `cut` column of the report)
CUTS = {
    "ChunkWriter<Hit,HIT_CHUNK>": {256},
    "ChunkWriter<Candidate,CAND_CHUNK>": {512},
    "BufferedWriter<Candidate>": {256, 2048},
    "BufferedWriter<RareAnchor>": {256, 2048},
    "BufferedWriter<uint32_t>": {256, 2048},
    "BufferedWriter<uint2,RARE_STAGE>": {256, 2048},
    "StagedChunkWriter<Candidate,CAND_STAGE>/64": {64},
    "StagedChunkWriter<Candidate,CAND_STAGE>/1024": {1024},
    "DomWriter/static/256": {256, 1024},
    "DomWriter/static/1024": {1024},
    "DomWriter/reserved/256": {256},
    "DomWriter/reserved/1024": {1024},
}
CASE = re.compile(r"^CASE (\S+) W=(\d+) cap=(\d+) counter=(\d+) cut=(\d+) (OK|FAIL: .*)$")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("list_writers") / "list_writers"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", str(CSRC), str(ROOT / "tests" / "hip" / "list_writers.hip"), "-o", str(exe)],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    cases = {}
    for line in r.stdout.splitlines():
        m = CASE.match(line)
        if m:
            cases.setdefault(m.group(1), []).append(dict(W=int(m.group(2)), cap=int(m.group(3)), counter=int(m.group(4)), cut=int(m.group(5)), verdict=m.group(6)))
    return r, cases


def test_harness_ran_to_its_end(report):
    r, cases = report
    done = re.search(r"^DONE cases=(\d+) failed=(\d+)$", r.stdout, re.M)
    assert done, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(done.group(1)) == sum(len(v) for v in cases.values())
    assert set(cases) == set(WRITERS), sorted(set(cases) ^ set(WRITERS))
    assert (r.returncode == 0) == (int(done.group(2)) == 0)


def test_harness_stage_sizes_are_k_anchors():
    # CAND_STAGE / RARE_STAGE live in k_anchor.hip, which the harness cannot include: its copies must be the same numbers
    src = (CSRC / "k_anchor.hip").read_text()
    m = re.search(r"constexpr uint32_t CAND_STAGE = (\d+), RARE_STAGE = (\d+);", src)
    h = re.search(r"constexpr uint32_t CAND_STAGE = (\d+), RARE_STAGE = (\d+);", (ROOT / "tests" / "hip" / "list_writers.hip").read_text())
    assert m and h and m.groups() == h.groups()
    for use in ("StagedChunkWriter<Candidate, CAND_STAGE>", "BufferedWriter<uint2, RARE_STAGE>"):
        assert use in src


@pytest.mark.parametrize("writer", WRITERS)
def test_writer_against_the_host_model(report, writer):
    r, cases = report
    mine = cases.get(writer)
    assert mine, r.stdout[-2000:] + r.stderr[-2000:]
    for c in mine:
        print(writer, c)
    bad = [c for c in mine if c["verdict"] != "OK"]
    assert not bad, bad
    for W in WAVES:
        caps = [c["cap"] for c in mine if c["W"] == W]
        demand = {c["counter"] for c in mine if c["W"] == W}
        assert len(demand) == 1, (W, demand)   # the demand does not depend on the capacity: counted past it
        d = demand.pop()
        assert d > 0
        # no overflow, exactly the demand, one less, nothing at all, and at least one capacity strictly inside the list
        assert caps[0] == d + 1000 and d in caps and d - 1 in caps and 0 in caps, (W, d, caps)
        assert any(0 < cap < d - 1 for cap in caps), (W, d, caps)
    cut = {c["cut"] for c in mine}
    assert CUTS[writer] <= cut, (CUTS[writer], cut)
