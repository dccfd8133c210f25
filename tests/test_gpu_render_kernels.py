"""GPU: the kernels of csrc/render.hip through their launch wrappers alone (csrc/render.h), against a sequential host model built
from csrc/render_core.h, at block capacities around and below the demand, with the payload table empty and filled.

tests/hip/render.hip holds the cases, the model and the comparison (read its head for what is asserted). It is compiled here, from
the test, with hipcc for gfx950 together with csrc/render.hip into pytest's temporary directory and run ONCE, as a child process with a
time limit: one process, sequential launches. Every test below reads that one run's report.

The contract these tests guard ("Rendered records"): the demand is counted past the capacity, nothing is stored at or
behind min(demand, capacity) or in front of the block, a block that fits is exact, the miss list counts past its capacity and never
writes past it, and both tiers of records and the cut fields are exercised.
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

CASES = ["tier_edges", "long_line", "many_ids", "all_negative", "compact_ipv4", "segments", "ipv6_fallback", "short_lines", "big_payload", "zero_records", "no_line_keys",
         "line_numbers", "many_records"]
LINE = re.compile(r"^(CASE|MISS|CROWDED|SWEEP|PIECES|LIMIT) (\S+) (.*?) (OK|FAIL: .*)$")


def constant(name):
    m = re.search(r"constexpr uint\d+_t %s = (\d+)" % name, (CSRC / "render.h").read_text())
    return int(m.group(1))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = tmp_path_factory.mktemp("render") / "render"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", str(CSRC), str(ROOT / "tests" / "hip" / "render.hip"), str(CSRC / "render.hip"),
                    "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    rows = {}
    for line in r.stdout.splitlines():
        m = LINE.match(line)
        if m:
            fields = {k: int(v) for k, v in (kv.split("=") for kv in m.group(3).split())}
            rows.setdefault((m.group(1), m.group(2)), []).append(dict(fields, verdict=m.group(4)))
    return r, rows


def test_harness_ran_to_its_end(report):
    r, rows = report
    done = re.search(r"^DONE cases=(\d+) failed=(\d+)$", r.stdout, re.M)
    assert done, r.stdout[-3000:] + r.stderr[-3000:]
    assert int(done.group(1)) == sum(len(v) for v in rows.values())
    assert {name for kind, name in rows if kind == "CASE"} == set(CASES)
    assert (r.returncode == 0) == (int(done.group(2)) == 0)


@pytest.mark.parametrize("case", CASES)
def test_block_against_the_host_model(report, case):
    r, rows = report
    mine = rows.get(("CASE", case))
    assert mine, r.stdout[-2000:] + r.stderr[-2000:]
    for c in mine:
        print(case, c)
    bad = [c for c in mine if c["verdict"] != "OK"]
    assert not bad, bad
    demand = {c["demand"] for c in mine}
    assert len(demand) == 1, demand   # counted past the capacity: the same at every capacity
    d = demand.pop()
    caps = [c["cap"] for c in mine]
    if case == "zero_records":
        assert d == 0 and mine[0]["records"] == 0 and caps == [0, 1]
    else:
        assert d > 0 and caps == [0, d - 1, d, d + 1, 2 * d], (d, caps)


@pytest.mark.parametrize("case", CASES)
def test_miss_list_against_the_host_model(report, case):
    """the table empty: the distinct data offsets of the case, whatever the capacity of the list; nothing behind the capacity"""
    r, rows = report
    mine = rows.get(("MISS", case))
    assert mine, r.stdout[-2000:] + r.stderr[-2000:]
    bad = [c for c in mine if c["verdict"] != "OK"]
    assert not bad, bad
    misses = {c["misses"] for c in mine}
    assert len(misses) == 1, misses
    n = misses.pop()
    caps = [c["cap"] for c in mine]
    if case in ("zero_records", "all_negative"):   # no record names a payload
        assert n == 0 and caps == [0]
    else:
        assert n > 1 and caps == [0, n - 1, n], (n, caps)


def test_every_tier_and_the_cut_fields_ran(report):
    _, rows = report
    short_max, piece = constant("RENDER_SHORT_MAX"), constant("RENDER_PIECE")
    assert (short_max, constant("RENDER_SHORT_IDS")) == (512, 8) and piece == 16384
    edges = rows[("CASE", "tier_edges")][0]
    assert (edges["short"], edges["long"]) == (3, 2)   # -1 and +0 and 8 ids are short; +1 and 9 ids are long
    long_line = rows[("CASE", "long_line")][0]
    # seven lines of 3 * RENDER_PIECE + 1 bytes with two records each: four pieces of the line per record, one piece of the hit (two for one hit)
    assert (long_line["short"], long_line["long"], long_line["pieces"]) == (2, 14, 14 * (4 + 1) + 1)
    big = rows[("CASE", "big_payload")][0]
    assert (big["short"], big["long"], big["pieces"]) == (3, 1, 2)   # RENDER_SHORT_TEXT bytes of text stay with a lane, more does not
    assert constant("RENDER_SHORT_TEXT") == 8192
    assert rows[("CASE", "many_ids")][0]["long"] == 1 and rows[("CASE", "all_negative")][0]["long"] == 1
    assert rows[("CASE", "no_line_keys")][0]["short"] == 1 and rows[("CASE", "no_line_keys")][0]["long"] == 2
    many = rows[("CASE", "many_records")][0]
    assert many["records"] > 2 * constant("RENDER_SCAN_CHUNK") and many["long"] == 4   # the prefix sum runs more than two workgroups
    assert sum(c[0]["short"] for (k, _), c in rows.items() if k == "CASE") > 0
    assert sum(c[0]["pieces"] for (k, _), c in rows.items() if k == "CASE") >= 3


def test_crowded_miss_set(report):
    """a set of two slots: lanes append without a claim; the list holds every offset of the case and nothing else"""
    _, rows = report
    mine = [(name, c) for (kind, name), v in rows.items() if kind == "CROWDED" for c in v]
    assert len(mine) == len(CASES) - 2   # every case that names a payload
    assert all(c["verdict"] == "OK" for _, c in mine), mine


def test_capacities_inside_records_and_16_byte_units(report):
    """a block that ends anywhere around a record boundary: nothing at or behind the capacity, the bytes in front exact"""
    _, rows = report
    mine = [(name, c) for (kind, name), v in rows.items() if kind == "SWEEP" for c in v]
    assert {name for name, _ in mine} >= {"many_records", "long_line", "tier_edges", "big_payload", "compact_ipv4"}
    assert all(c["verdict"] == "OK" and c["caps"] >= 81 for _, c in mine), mine


def test_piece_arrays_one_slot_short(report):
    """the pass reports it, counts the slots it needs and stores nothing in the block or behind the arrays"""
    _, rows = report
    mine = [(name, c) for (kind, name), v in rows.items() if kind == "PIECES" for c in v]
    assert {name for name, _ in mine} >= {"tier_edges", "long_line", "many_ids", "many_records"}
    assert all(c["verdict"] == "OK" and c["pieces"] == c["cap"] + 1 for _, c in mine), mine


def test_demand_above_the_limit_is_too_large(report):
    _, rows = report
    mine = [(name, c) for (kind, name), v in rows.items() if kind == "LIMIT" for c in v]
    assert len(mine) == len(CASES) - 1   # every case with records
    assert all(c["verdict"] == "OK" for _, c in mine), mine
