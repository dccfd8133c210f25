"""GPU: whole-line queries (csrc/whole_lines.hip, matchy_scanner_set_whole_lines / Scanner.set_whole_lines): every line of a buffer is
one query, answered like a single Database::lookup.

The model is tests/whole_lines_cases.py: a Python line split and one single query per line through the oracle and through the
library's host path (Database.query_json), which must agree; the embedded-IPv4 lines are also written out by hand. A scan is compared
as a whole: the records (span, type, kind, prefix, ids), the data they render, and the four counters of the mode."""
import ctypes
import gzip
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tally_cases as T         # noqa: E402
import whole_lines_cases as W   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = W.ROOT
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    return _hip


def on_device(data):
    dptr = ctypes.c_void_p()
    assert hip().hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(len(data) + 64)) == 0
    if data:
        assert hip().hipMemcpy(dptr, data, ctypes.c_size_t(len(data)), 1) == 0
    return dptr


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


class Case:
    """one database, open in the library and in the oracle, with a scanner in whole-line mode and the models of the lists asked of it"""

    def __init__(self, M, oracle, entries, ci=False):
        self.M = M
        self.blob = W.build_blob(entries, case_insensitive=ci)
        self.db = M.Database(self.blob)
        self.odb = W.Memo(oracle.Database(self.blob))
        self.host = W.memoized(W.host_from_db(self.db))
        self.sc = M.Scanner(self.db)
        self.sc.set_whole_lines(True)
        self._models = {}

    def model(self, buf):
        if buf not in self._models:
            self._models[buf] = W.model(self.odb, self.host, buf)
        return self._models[buf]

    def close(self):
        self.sc.close()
        self.odb.close()
        self.db.close()


@pytest.fixture(scope="module")
def cases(M, oracle):
    """the databases of the tests, built once: the rule database case-sensitive and not, the same with a pure-wildcard glob of three
    characters, and one whose only glob is '*' (every string query hits, the empty one included)"""
    out = {"cs": Case(M, oracle, W.rule_entries()), "ci": Case(M, oracle, W.rule_entries(), ci=True),
           "wild": Case(M, oracle, W.rule_entries(wild="???")), "star": Case(M, oracle, [("*", {"k": "any"}), ("192.0.2.7", {"k": "host"})])}
    yield out
    for c in out.values():
        c.close()


def check_records(r, buf, recs, sort=False):
    hits = r.hits()
    rendered = [json.loads(x) for x in r.ndjson(buf)]
    if sort:
        order = sorted(range(len(hits)), key=lambda i: hits[i]["start"])
        hits, rendered = [hits[i] for i in order], [rendered[i] for i in order]
    assert [(h["start"], h["end"]) for h in hits] == [(w["start"], w["end"]) for w in recs]
    for h, j, w in zip(hits, rendered, recs):
        q = buf[w["start"]:w["end"]]
        assert (h["type"], h["kind"], h["prefix_len"]) == (w["type"], w["kind"], w["prefix_len"]), (q, h, w)
        assert j["matched_text"].encode() == q
        if w["kind"] == "ip":
            assert j["data"] == w["data"][0] and j["cidr"] == w["cidr"] and j["prefix_len"] == w["prefix_len"], (q, j, w)
        else:
            assert j.get("data", []) == w["data"], (q, j, w)
            if w["ids"] is not None:
                assert h["ids"] == w["ids"] and j["pattern_count"] == len(w["ids"]), (q, h, w)
            assert len(h["offs"]) == len(h["ids"])


def scan_and_check(c, buf):
    recs, ctr = c.model(buf)
    r = c.sc.scan(buf)
    try:
        check_records(r, buf, recs)
        assert c.sc.whole_lines_counters() == ctr
        assert r.lines == buf.count(b"\n") and r.candidates == ctr["address"] + ctr["string"] and r.n_hits == len(recs)
    finally:
        r.close()
    return recs, ctr


# ------------------------------------------------------------------------------------------------ 1. every rule once
@pytest.mark.parametrize("name", ["cs", "ci", "wild"])
def test_every_rule_once(cases, name):
    c = cases[name]
    buf = W.rule_list()
    recs, ctr = scan_and_check(c, buf)
    found = {buf[r["start"]:r["end"]] for r in recs}
    assert {b"192.0.2.7", b"fe80::1", b"::ffff:192.0.2.1", b"64:ff9b::192.0.2.33", b"evil.com", b"foo.com.", b"both.evil.org", b"1.2.3", "münchen.example".encode()} <= found
    assert not ({b"01.2.3.4", b"1.2.3.4/32", b" 1.2.3.4", b"1.2.3.4 ", b"fe80::1%eth0", W.HEX47, b"good.com"} & found)
    assert (b"EXAMPLE.COM" in found) == (name == "ci") and (b"abc" in found) == (name == "wild") and b"ab" not in found
    assert ctr["invalid_utf8"] == 0 and ctr["queries"] == len(W.RULE_QUERIES) + 1


# ------------------------------------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("buf", [b"", b"\n", b"a", b"a\n", b"\n\n\n", b"\n" * 70 + b"192.0.2.7\n", b"a\nbb\n192.0.2.7"],
                         ids=["empty", "one-newline", "a", "a-newline", "three-newlines", "70-empty-lines", "unterminated"])
def test_cuts(cases, buf):
    c = cases["star"]   # every string line is a hit, the empty ones too: the records ARE the line cuts
    recs, ctr = scan_and_check(c, buf)
    assert [(r["start"], r["end"]) for r in recs] == W.split_lines(buf)
    assert ctr["queries"] == len(W.split_lines(buf))


# ------------------------------------------------------------------------------------------------ 3. boundaries of the kernel's units
@pytest.mark.parametrize("unit_name", ["WL_LANE_BYTES", "WL_TILE", "WL_WG_CHUNK"])
def test_boundaries_of_the_kernel_units(cases, unit_name):
    unit = W.kernel_units()[unit_name]
    c = cases["cs"]
    for boundary in (unit, 3 * unit) if unit >= 64 else (4 * unit, 7 * unit, 64 * unit + unit):
        for name, buf in W.boundary_lists(unit, boundary).items():
            recs, ctr = scan_and_check(c, buf)
            assert recs, (unit_name, boundary, name)
            if name.startswith("bad_"):
                assert ctr["invalid_utf8"] == 1, (unit_name, boundary, name)
            if name == "long_line":
                assert any(r["end"] - r["start"] > 2 * unit for r in recs), (unit_name, boundary)


# ------------------------------------------------------------------------------------------------ 4. invalid UTF-8
@pytest.mark.parametrize("bad", W.BAD_SEQUENCES, ids=[b.hex() for b in W.BAD_SEQUENCES])
def test_invalid_utf8_is_counted_and_not_looked_up(cases, bad):
    buf = W.invalid_list(bad)
    for c in (cases["cs"], cases["star"]):   # with '*' every line that is looked up hits: an invalid line that was would show
        recs, ctr = scan_and_check(c, buf)
        assert ctr["invalid_utf8"] == 3 and ctr["queries"] == 7
    assert [buf[r["start"]:r["end"]] for r in cases["cs"].model(buf)[0]] == [b"evil.com", b"192.0.2.7", "€evil".encode(), b"evil.com"]


# ------------------------------------------------------------------------------------------------ 5. capacity
def test_capacity_every_line_a_hit_then_the_rule_list(M, oracle):
    c = Case(M, oracle, W.rule_entries() + [("a", {"k": "a"})])
    try:
        n = 60000
        buf = b"a\n" * n   # 12 x the len / 24 estimate of the extraction path, 4 x the mode's own
        r = c.sc.scan(buf)
        try:
            hits = r.hits()
            assert len(hits) == n and r.n_hits == n
            assert [h["start"] for h in hits] == list(range(0, 2 * n, 2)) and all(h["end"] == h["start"] + 1 for h in hits)
            one = c.model(b"a\n")[0][0]
            assert all((h["type"], h["kind"], h["ids"]) == (one["type"], one["kind"], one["ids"]) for h in hits)
            assert c.sc.whole_lines_counters() == dict(queries=n, address=0, string=n, invalid_utf8=0)
        finally:
            r.close()
        scan_and_check(c, W.rule_list())
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 6. a long line
def child(case, env_extra=None, timeout=120):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "whole_lines_cases.py"), case], capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout), p.stderr


def test_a_long_line_costs_no_lane_a_walk(oracle):
    """in a process of its own: a lane that walked a line would make this slow, not wrong — the time limit of the child is the guard"""
    out, _ = child("long", timeout=60)
    buf = W.long_list()
    spans = W.split_lines(buf)
    got = [(h[0], h[1]) for h in out["hits"]]
    assert got == [spans[0], spans[1], spans[2], spans[4]]   # the line of colons has no hit
    assert spans[1][1] - spans[1][0] == W.LONG_BYTES
    odb = oracle.Database(W.build_blob(W.long_entries()))
    try:
        for h in out["hits"]:
            want = W.oracle_answer(odb, buf[h[0]:h[1]])
            assert (h[3], h[4], h[5]) == (want["kind"], want["prefix_len"], want["ids"]), h[:2]
    finally:
        odb.close()
    assert out["counters"] == dict(queries=5, address=1, string=4, invalid_utf8=0)


# ------------------------------------------------------------------------------------------------ 7. entries
def test_all_entries_give_the_same_records(cases, M):
    c = cases["cs"]
    buf = W.rule_list()
    recs, ctr = c.model(buf)
    want = None
    r = c.sc.scan(buf)
    try:
        check_records(r, buf, recs)
        want = sorted(W.hit_rows(r))
    finally:
        r.close()
    # the host buffer in three pieces (the piece size is read once per process)
    out, err = child("pieces", {"MATCHY_AMD_HOST_PIECE_BYTES": str(len(buf) // 3 + 1), "MATCHY_AMD_TRACE": "1"})
    assert err.count("scan_host piece") >= 3, err[-2000:]
    assert sorted(out["hits"]) == want and out["counters"] == ctr and out["lines"] == buf.count(b"\n")
    dptr = on_device(buf)
    try:
        for mode in (1, 3):   # records as the kernels left them / sorted on the GPU
            r = c.sc.scan_device(dptr.value, len(buf), 0, mode)
            try:
                check_records(r, buf, recs, sort=(mode == 1))
                assert sorted(W.hit_rows(r)) == want and c.sc.whole_lines_counters() == ctr
            finally:
                r.close()
        c.sc.submit_device(dptr.value, len(buf), 0, 3)
        r = c.sc.wait()
        try:
            check_records(r, buf, recs)
            assert sorted(W.hit_rows(r)) == want
        finally:
            r.close()
    finally:
        hip().hipFree(dptr)
    ms = M.MultiScanner(c.db, devices=(0, 0))
    try:
        ms.set_whole_lines(True)
        r = ms.scan(buf, batch_bytes=len(buf) // 4)
        try:
            check_records(r, buf, recs)
            assert sorted(W.hit_rows(r)) == want and r.lines == buf.count(b"\n")
        finally:
            r.close()
    finally:
        ms.close()


# ------------------------------------------------------------------------------------------------ 8. line context, tally
def test_line_context_numbers_are_query_numbers(cases, M):
    c = cases["cs"]
    buf = W.repeats_list()
    recs, _ = c.model(buf)
    ends = [i for i, b in enumerate(buf) if b == 0x0A]
    c.sc.set_line_context(True)
    try:
        r = c.sc.scan(buf)
        try:
            check_records(r, buf, recs)
            lines = r.line_records
            assert [ln[0] for ln in lines] == [w["line"] for w in recs]
            assert [ln[1] for ln in lines] == [w["start"] for w in recs]
            assert [ln[2] for ln in lines] == [ends[w["line"]] for w in recs]   # a '\r' in front of the '\n' belongs to the line
            assert r.lines_with_matches == len(recs)
            numbered = [json.loads(x) for x in r.ndjson_lines_text(buf, "list", 1000).decode().splitlines()]
            assert [j["line_number"] for j in numbered] == [1000 + w["line"] + 1 for w in recs]
        finally:
            r.close()
    finally:
        c.sc.set_line_context(False)
    # across the batches of the multi-device scanner the numbers continue
    ms = M.MultiScanner(c.db, devices=(0, 0))
    try:
        ms.set_whole_lines(True)
        ms.set_line_context(True)
        r = ms.scan(buf, batch_bytes=len(buf) // 5)
        try:
            check_records(r, buf, recs)
            assert [ln[0] for ln in r.line_records] == [w["line"] for w in recs]
        finally:
            r.close()
    finally:
        ms.close()


def test_tally_counts_hits_per_distinct_query_text(cases, M):
    c = cases["cs"]
    buf = W.repeats_list()
    recs, _ = c.model(buf)
    want = W.model_tally(recs, buf)
    sc = M.Scanner(c.db)
    try:
        sc.set_whole_lines(True)
        sc.set_tally(True)
        for part in (buf, buf):
            r = sc.scan(part)
            r.close()
        t = sc.tally()
        assert [(text, typ, n) for text, typ, n in t] == [(text, typ, 2 * n) for text, typ, n in T.ordered(want)]
        assert t.distinct == len(want) and t.matches == 2 * len(recs)
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_combinations_the_mode_does_not_have_are_refused(cases, M):
    c = cases["cs"]
    buf = W.rule_list()
    sc = M.Scanner(c.db)
    dptr = on_device(buf)
    try:
        sc.set_whole_lines(True)
        assert sc.whole_lines_enabled()

        def refused(what, run):
            with pytest.raises(RuntimeError) as e:
                run()
            assert "whole-line mode and " + what in str(e.value) and "-5" in str(e.value), str(e.value)
            assert "whole-line mode and " + what in M.last_error()

        for run in (lambda: sc.scan(buf), lambda: sc.scan_device(dptr.value, len(buf), 0, 1), lambda: sc.submit_device(dptr.value, len(buf), 0, 1)):
            sc.set_segments([0, 10])
            refused("segments", run)
            sc.set_render(0, source="list")
            refused("rendered records", run)
            sc.set_hit_lines(True)
            refused("hit lines", run)
            sc.set_hit_lines(False)
        refused("gz scans", lambda: sc.scan_gz([gzip.compress(b"evil.com\n")]))
        # a refusal drops the pending table and parameters: the scanner answers the list as before
        r = sc.scan(buf)
        try:
            check_records(r, buf, c.model(buf)[0])
        finally:
            r.close()
        ms = M.MultiScanner(c.db, devices=(0,))
        try:
            ms.set_whole_lines(True)
            ms.set_hit_lines(True)
            with pytest.raises(RuntimeError) as e:
                ms.scan(buf)
            assert "whole-line mode and hit lines" in str(e.value)
        finally:
            ms.close()
    finally:
        hip().hipFree(dptr)
        sc.close()


# ------------------------------------------------------------------------------------------------ 10. mode off
def test_mode_off_the_same_scanner_extracts_again(M, oracle):
    blob = T.build_blob(T.every_type_entries())
    data = T.every_type_log()
    odb = oracle.Database(blob)
    want, _, _ = odb.scan(data, want_json=False)
    odb.close()
    db = M.Database(blob)
    sc = M.Scanner(db)
    try:
        sc.set_whole_lines(True)
        r = sc.scan(data)
        n_mode = r.n_hits
        r.close()
        sc.set_whole_lines(False)
        assert not sc.whole_lines_enabled()
        r = sc.scan(data)
        try:
            got = r.hits()
        finally:
            r.close()
        key = lambda h: (h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]))   # noqa: E731
        assert sorted(map(key, got)) == sorted(map(key, want)) and len(got) != n_mode
    finally:
        sc.close()
        db.close()
