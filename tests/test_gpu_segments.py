"""GPU: segmented scans (matchy_scanner_set_segments, segments.hip) through every scan entry.

Oracles. The expected records of a packed scan are the records of each segment scanned ALONE through matchy_scanner_scan without
segments — the existing, pinned path — shifted by the segment's start; the match set also goes against the CPU oracle. The segment of
every record and the per-segment table go against the host model of tests/segment_cases.py (numpy.searchsorted and counting)."""
import ctypes
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import segment_cases as S
import test_gpu_line_context as LC

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
INVALID_PARAM = -5
hip, on_device = LC.hip, LC.on_device


def key(h):
    return (h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]))


class Env:
    """databases, scanners and the per-segment reference scans shared by the cases of this module"""

    def __init__(self):
        import matchy_amd as M
        self.M = M
        self.blob, self.blob4 = S.blob(), S.blob(ip_only=True, every_address=True)
        self.db, self.db4 = M.Database(self.blob), M.Database(self.blob4)
        self.sc, self.sc4 = M.Scanner(self.db), M.Scanner(self.db4)
        self.alone = {False: M.Scanner(self.db), True: M.Scanner(self.db4)}
        self.ms = M.MultiScanner(self.db, devices=(0, 0))
        self._alone_hits = {False: {}, True: {}}
        self._shapes = None

    def shapes(self):
        if self._shapes is None:
            self._shapes = S.shapes(self.M.LINE_TILE, self.M.LINE_SCAN_CHUNK)
        return self._shapes

    def expected(self, buf, starts, every=False):
        """the records of every segment scanned alone (once per distinct content), shifted by its start"""
        cache, out = self._alone_hits[every], []
        for start, seg in zip(starts, S.cut(buf, starts)):
            if seg not in cache:
                r = self.alone[every].scan(seg)
                assert not r.has_segments
                cache[seg] = r.hits()
                r.close()
            for h in cache[seg]:
                out.append(key(dict(h, start=h["start"] + start, end=h["end"] + start)))
        return out

    def close(self):
        for x in (self.ms, self.sc, self.sc4, *self.alone.values(), self.db, self.db4):
            x.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def read(res):
    """(hit starts, segment of every hit, table) of a result; compact records first, like hits()"""
    raw, dev = res._raw, res.on_device
    addr = lambda p: ctypes.cast(p, ctypes.c_void_p).value or 0
    recs = LC._array(addr(raw.hits), raw.n_hits if raw.hits else 0, LC.REC, dev)
    c4 = LC._array(addr(raw.ip4_hits), 2 * raw.n_ip4_hits if raw.ip4_hits else 0, np.dtype("<u4")).reshape(-1, 2)[:, 0]
    sa = res._segment_arrays()
    assert sa is not None
    of = LC._array(sa[0], len(recs), np.dtype("<u4"), dev)
    of4 = LC._array(sa[1], len(c4), np.dtype("<u4"))
    return np.concatenate([c4, recs["start"]]).astype(np.int64), np.concatenate([of4, of]).astype(np.int64), table_of(res)


def table_of(res):
    return [(s["start"], s["len"], s["hits"], s["line_base"], s["lines"], s["lines_with_matches"]) for s in res.segments]


def check(res, buf, starts, lines, what, n_expected):
    assert res.has_segments, what
    hit_starts, of, table = read(res)
    assert len(hit_starts) == n_expected == len(of), (what, len(hit_starts), n_expected)
    want_of = S.segment_of(starts, hit_starts)
    bad = np.flatnonzero(of != want_of)
    assert len(bad) == 0, (what, "first wrong record", int(hit_starts[bad[0]]), int(of[bad[0]]), int(want_of[bad[0]]), len(bad))
    want = S.table_model(buf, starts, hit_starts, lines)
    wrong = [i for i in range(len(want)) if i >= len(table) or table[i] != want[i]]
    assert len(table) == len(want) and not wrong, (what, "first wrong segment", wrong[0], table[wrong[0]] if wrong[0] < len(table) else None, want[wrong[0]], len(wrong))
    return table


def through_every_entry(env, oracle, name):
    buf, starts = env.shapes()[name]
    text = buf.tobytes()
    sc, sc4 = env.sc, env.sc4
    want, want4 = env.expected(buf, starts), env.expected(buf, starts, every=True)
    odb = oracle.Database(env.blob)
    ohits, _, _ = odb.scan(text, want_json=False)
    odb.close()
    assert sorted((h["start"], h["end"], h["type"]) for h in ohits) == sorted(k[:3] for k in want), (name, "oracle")
    assert len(want) > 0 and len(want4) > 0, name
    dptr = on_device(buf)
    keep = ctypes.create_string_buffer(text, len(text))
    try:
        for lines in (False, True):
            for s in (sc, sc4):
                s.set_line_context(lines)
            env.ms.set_line_context(lines)
            # host buffer: canonical order, owned arrays
            what = (name, lines, "scan")
            sc.set_segments(starts)
            r = sc.scan(text)
            assert [key(h) for h in r.hits()] == want, what
            table = check(r, buf, starts, lines, what, len(want))
            if lines:   # the line of a hit inside its input
                of, rel = r.segment_of, S.segment_of(starts, [h["start"] for h in r.hits()])
                nl = np.flatnonzero(buf == 10)
                for (line, _, _), s_, h in zip(r.line_records, of, r.hits()):
                    assert line - table[s_][3] == int(np.searchsorted(nl, h["start"], "left") - np.searchsorted(nl, starts[s_], "left")), what
                assert list(rel) == of
            r.close()
            # one-shot: the next scan has no segment block
            r = sc.scan(text)
            assert not r.has_segments and r.segments is None and [key(h) for h in r.hits()] == want, what
            assert env.M.lib().matchy_scan_result_segments(ctypes.byref(r._raw), None, None, None, None) == INVALID_PARAM, what
            r.close()
            for mode in (0, 1, 3, 4):
                what = (name, lines, "scan_device", mode)
                sc.set_segments(starts)
                r = sc.scan_device(dptr.value, len(text), fetch_mode=mode)
                assert r.n_hits == len(want), what
                if mode == 0:   # counters only: no per-record array crosses the bus, the table still does
                    assert r.has_segments and r.segment_of_ptr == 0 and table_of(r) == table, what
                else:
                    assert r.on_device == (mode == 4), what
                    if mode != 4:
                        got = [key(h) for h in r.hits()]
                        assert (got == want) if mode == 3 else (sorted(got) == sorted(want)), what
                    assert check(r, buf, starts, lines, what, len(want)) == table, what
                r.close()
            # compact records of a database that answers every address: a second index array parallel to ip4_hits
            what = (name, lines, "compact")
            sc4.set_segments(starts)
            r = sc4.scan_device(dptr.value, len(text), fetch_mode=9)
            assert r.n_ip4_hits > 0 and r.n_ip4_hits == r.n_hits == len(want4), what
            assert sorted(key(h) for h in r.hits()) == sorted(want4), what
            check(r, buf, starts, lines, what, len(want4))
            r.close()
            # submit / wait: the table is read at submit
            what = (name, lines, "submit/wait")
            sc.set_segments(starts)
            sc.submit_device(dptr.value, len(text), fetch_mode=1)
            sc.set_segments([0, 0])   # belongs to the scan after this one ...
            r = sc.wait()
            assert sorted(key(h) for h in r.hits()) == sorted(want), what
            assert check(r, buf, starts, lines, what, len(want)) == table, what
            r.close()
            sc.set_segments([])       # ... and is cleared
            r = sc.scan_device(dptr.value, len(text), fetch_mode=1)
            assert not r.has_segments, what
            r.close()
            # a worker of the multi-device scanner
            what = (name, lines, "multi")
            env.ms.submit_segments_ptr(ctypes.addressof(keep), len(text), starts)
            b = env.ms.next(want_hits=True)
            assert [key(h) for h in b["hits"]] == want, what
            assert [tuple(s[k] for k in ("start", "len", "hits", "line_base", "lines", "lines_with_matches")) for s in b["segments"]] == table, what
            assert b["segment_of"] == list(S.segment_of(starts, [h["start"] for h in b["hits"]])), what
            env.ms.submit_ptr(ctypes.addressof(keep), len(text))
            assert "segments" not in env.ms.next(), what
    finally:
        for s in (sc, sc4):
            s.set_line_context(False)
        env.ms.set_line_context(False)
        hip().hipFree(dptr)


SHAPES = ["n1", "n2", "lines_1023", "lines_1024", "lines_1025", "lines_2049", "empties", "one_byte", "edge_hits", "tile_starts",
          "unterminated_last", "unterminated_only", "skew", "crlf"]


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_through_every_entry(env, oracle, name):
    through_every_entry(env, oracle, name)


def test_shapes_hold_what_they_are_named_for(env):
    sh = env.shapes()
    T, C = env.M.LINE_TILE, env.M.LINE_SCAN_CHUNK
    for n in (1023, 1024, 1025, 2049):
        buf, starts = sh[f"lines_{n}"]
        assert len(starts) == n and 25000 < len(buf) * 2049 // n < 40000
    _, st = sh["tile_starts"]
    assert {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, C * T - 1, C * T, C * T + 1} <= set(st)
    buf, st = sh["empties"]
    assert st[0] == st[1] == st[2] == 0 and st[-1] == len(buf) and any(st[i] == st[i + 1] == st[i + 2] == st[i + 3] for i in range(3, len(st) - 3))
    buf, st = sh["edge_hits"]
    want = env.expected(buf, st)
    assert any(k[0] in st for k in want) and any(buf[k[1]] == 10 for k in want if k[1] < len(buf))
    buf, st = sh["skew"]
    table = S.table_model(buf, st, [k[0] for k in env.expected(buf, st)], False)
    assert len(st) == 501 and sorted(t[2] for t in table)[-2:] == [0, 6000]


def test_counts_only_table_equals_the_sorted_fetch(env):
    buf, starts = env.shapes()["lines_2049"]
    dptr = on_device(buf)
    try:
        for lines in (False, True):
            env.sc.set_line_context(lines)
            tables = []
            for mode in (3, 0):
                env.sc.set_segments(starts)
                r = env.sc.scan_device(dptr.value, len(buf), fetch_mode=mode)
                tables.append(table_of(r))
                r.close()
            assert tables[0] == tables[1] and sum(t[2] for t in tables[0]) > 1000
            assert (sum(t[4] for t in tables[0]) == 2049) == lines
    finally:
        env.sc.set_line_context(False)
        hip().hipFree(dptr)


def test_ndjson_with_per_segment_sources(env):
    """line_bases NULL: the bytes of matchy_scan_result_to_ndjson per segment; with line_bases: those of _to_ndjson_lines, numbered
    inside the segment"""
    a = b"x 10.1.2.3 y\nz evil.example.com and www.bad.example.org\n\n192.0.2.7\n"
    b = b"second \"file\" 192.0.2.7\nnothing\n198.51.100.1 evil.example.com\n"
    segs = [a, b"", b, b"no hits\n", a, b"tail 10.1.2.9"]
    names = ["a.log", "empty", 'dir/"b".log', "none", "a again", "tail\\.log"]
    buf, starts = S.pack(segs)
    text = buf.tobytes()
    sc, alone = env.sc, env.alone[False]
    for lines in (False, True):
        sc.set_line_context(lines)
        alone.set_line_context(lines)
        sc.set_segments(starts)
        r = sc.scan(text)
        parts = []
        for seg, name in zip(segs, names):
            ra = alone.scan(seg)
            parts.append(ra.ndjson_lines_text(seg, name, 7, True) if lines else ra.ndjson_text(seg, name))
            ra.close()
        got = r.ndjson_segments_text(text, names, [7] * len(segs), True) if lines else r.ndjson_segments_text(text, names)
        assert got == b"".join(parts) and got.count(b"\n") == r.n_hits > 8, lines
        if not lines:
            with pytest.raises(RuntimeError):
                r.ndjson_segments_text(text, names, [0] * len(segs))   # line numbers of a scan without line context
        r.close()
        r = sc.scan(text)
        with pytest.raises(RuntimeError):
            r.ndjson_segments_text(text, names)                        # a scan without segments
        r.close()
    sc.set_line_context(False)
    alone.set_line_context(False)


# ------------------------------------------------------------------------------------------------ rejected tables
def test_rejected_tables_leave_the_scanner_usable(env):
    """Refused on the host before anything is launched, or by the one-byte check of the segment pass at validated offsets."""
    M = env.M
    buf, good = env.shapes()["edge_hits"]
    text = buf.tobytes()
    middle = list(good)
    middle[2] -= 3                                    # segment 1 now ends in front of its '\n'
    bad_tables = {"starts[0] != 0": ([1] + good[1:], "starts[0]"), "a decreasing pair": ([0, good[2], good[1]] + good[3:], "segment 2"),
                  "a start beyond len": (good + [len(text) + 1], "segment %d" % len(good)), "a middle segment without a final newline": (middle, "segment 1 ")}
    fresh, used = M.Scanner(env.db), M.Scanner(env.db)
    dptr = on_device(buf)
    try:
        r = fresh.scan(text)
        want = [key(h) for h in r.hits()]
        r.close()
        r = fresh.scan_device(dptr.value, len(text), fetch_mode=3)
        want_dev = [key(h) for h in r.hits()]
        r.close()
        for what, (table, names) in bad_tables.items():
            for lines in (False, True):
                used.set_line_context(lines)
                for entry in ("scan", "scan_device", "submit/wait"):
                    used.set_segments(table)
                    with pytest.raises(RuntimeError) as e:
                        if entry == "scan":
                            used.scan(text)
                        elif entry == "scan_device":
                            used.scan_device(dptr.value, len(text), fetch_mode=1)
                        else:
                            used.submit_device(dptr.value, len(text), fetch_mode=1)
                            used.wait()
                    assert f"rc={INVALID_PARAM}" in str(e.value), (what, entry, str(e.value))
                    assert names in str(e.value) and "segments:" in str(e.value), (what, entry, str(e.value))
                    # the table was consumed; the same scanner's next plain scan returns exactly what a fresh scanner returns
                    r = used.scan(text)
                    assert not r.has_segments and [key(h) for h in r.hits()] == want, (what, entry)
                    r.close()
                    r = used.scan_device(dptr.value, len(text), fetch_mode=3)
                    assert not r.has_segments and [key(h) for h in r.hits()] == want_dev, (what, entry)
                    r.close()
        # ... and a good table still works on it
        used.set_segments(good)
        r = used.scan(text)
        check(r, buf, good, True, "good after bad", len(want))
        r.close()
    finally:
        hip().hipFree(dptr)
        fresh.close(); used.close()


# ------------------------------------------------------------------------------------------------ further cases
def test_smaller_segmented_scan_after_a_larger_one(env):
    M = env.M
    big, big_starts = env.shapes()["lines_2049"]
    small, small_starts = env.shapes()["edge_hits"]
    used = M.Scanner(env.db)
    used.set_line_context(True)
    d_big, d_small = on_device(big), on_device(small)
    try:
        for mode in (1, 3, 4):
            used.set_segments(big_starts)
            r = used.scan_device(d_big.value, len(big), fetch_mode=mode)
            check(r, big, big_starts, True, ("large", mode), len(env.expected(big, big_starts)))
            r.close()
            used.set_segments(small_starts)
            r = used.scan_device(d_small.value, len(small), fetch_mode=mode)
            check(r, small, small_starts, True, ("small after large", mode), len(env.expected(small, small_starts)))
            r.close()
        used.set_segments(big_starts)
        r = used.scan(big.tobytes())
        check(r, big, big_starts, True, "large, host", len(env.expected(big, big_starts)))
        r.close()
        used.set_segments(small_starts)
        r = used.scan(small.tobytes())
        check(r, small, small_starts, True, "small after large, host", len(env.expected(small, small_starts)))
        r.close()
    finally:
        hip().hipFree(d_big); hip().hipFree(d_small)
        used.close()


def _alternating_cases(T):
    """a log of three tiles and a bit with hits in all three of its segments, and one of 100 bytes with two segments and two hits"""
    L = 3 * T + 40
    big = LC.make_log(L, [(5, LC.IP), (600, LC.DOM), (T + 3, LC.DOM), (2 * T + 9, LC.IP), (L - 9, LC.IP)], [500, T - 1, T + 500, 2 * T + 4, 2 * T + 600])
    small = LC.make_log(100, [(3, LC.IP), (60, LC.DOM)], [49, 99])
    return (big, [0, T, 2 * T + 5]), (small, [0, 50])


@pytest.mark.parametrize("entry", ["scan_device", "scan"])
def test_line_context_switched_between_segmented_scans(env, entry):
    """One scanner, a table in front of every scan, line context on / off / on / off over a larger and a smaller log: the segment pass
    reads the prefix array and the distinct-line set of the line context of ITS fetch, or none. Every scan equals the same scan on a
    fresh scanner and the host model; without line context the three line figures are 0 (a stale prefix array or set would show)."""
    M = env.M
    (big, big_starts), (small, small_starts) = _alternating_cases(M.LINE_TILE)
    assert len(big) == 3 * M.LINE_TILE + 40 and len(small) == 100
    assert [t[2] for t in S.table_model(big, big_starts, [k[0] for k in env.expected(big, big_starts)], False)] == [2, 1, 2]
    assert [t[2] for t in S.table_model(small, small_starts, [k[0] for k in env.expected(small, small_starts)], False)] == [1, 1]
    used = M.Scanner(env.db)
    dptrs = {id(b): on_device(b) for b in (big, small)}

    def run(sc, buf, starts, lines):
        sc.set_line_context(lines)
        sc.set_segments(starts)
        return sc.scan(buf.tobytes()) if entry == "scan" else sc.scan_device(dptrs[id(buf)].value, len(buf), fetch_mode=3)
    try:
        for step, (lines, (buf, starts)) in enumerate([(True, (big, big_starts)), (False, (small, small_starts)), (True, (small, small_starts)),
                                                        (False, (big, big_starts))]):
            what = (entry, step, lines)
            fresh = M.Scanner(env.db)
            try:
                r, rf = run(used, buf, starts, lines), run(fresh, buf, starts, lines)
                hit_starts, of, table = read(r)
                f_starts, f_of, f_table = read(rf)
                assert list(hit_starts) == list(f_starts) and list(of) == list(f_of) and table == f_table, what
                assert r.has_lines == rf.has_lines == lines and r.lines_with_matches == rf.lines_with_matches, what
                assert (r.lines_with_matches is None) if not lines else (r.lines_with_matches == sum(t[5] for t in table) > 0), what
                check(r, buf, starts, lines, what, len(env.expected(buf, starts)))
                if not lines:
                    assert all(t[3:] == (0, 0, 0) for t in table), what
                r.close(); rf.close()
            finally:
                fresh.close()
    finally:
        for d in dptrs.values():
            hip().hipFree(d)
        used.close()


def _child(case, env_extra):
    e = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "segment_cases.py"), case], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout), p.stderr


def _check_child(got, buf, starts):
    hit_starts = got["starts"]
    assert got["segment_of"] == list(S.segment_of(starts, hit_starts))
    assert [tuple(t) for t in got["table"]] == S.table_model(buf, starts, hit_starts, True)


def test_regrown_lists_count_once():
    """a fresh scanner whose final_ list is over, forced the way tests/test_gpu_overflow.py forces it: the batch is scanned again, the
    segment passes run once behind the last rescan"""
    buf, starts = S.pack(S.regrow_segments())
    got, err = _child("regrow", {"MATCHY_AMD_TRACE": "1"})
    assert re.search(r"work buffers overflow \(attempt 0\): regrow and rescan:.* final_ \d+>\d+", err), err[-2000:]
    assert got["n_hits"] == 60000 and sum(t[2] for t in got["table"]) == 60000
    _check_child(got, buf, starts)


def test_host_pieces_with_segments_straddling_them():
    """MATCHY_AMD_HOST_PIECE_BYTES of a few hundred KiB: scan() cuts the buffer into pieces at line ends, segments of 70 000 bytes
    straddle them; indices are those of the caller's table, line_base is taken in the caller's buffer, the figures add up"""
    import matchy_amd as M
    buf, starts = S.pieces_case(M, False)
    got, err = _child("pieces", {"MATCHY_AMD_HOST_PIECE_BYTES": str(S.PIECE_BYTES), "MATCHY_AMD_TRACE": "1"})
    assert err.count("scan_host piece") >= 6
    assert got["n_hits"] > 30
    _check_child(got, buf, starts)


def test_runs_of_empty_segments_exactly_at_the_piece_cuts():
    """equal starts in front of the first byte and exactly where scan_host cuts: every one of them gets the line_base of its position"""
    import matchy_amd as M
    buf, starts = S.pieces_case(M, True)
    cuts = S.piece_cuts(buf)
    assert starts[:3] == [0, 0, 0] and starts.count(cuts[0]) >= 3 and starts.count(cuts[1]) >= 2 and cuts[3] in starts
    got, err = _child("pieces_cut", {"MATCHY_AMD_HOST_PIECE_BYTES": str(S.PIECE_BYTES), "MATCHY_AMD_TRACE": "1"})
    sizes = [int(x) for x in re.findall(r"scan_host piece (\d+) B", err)]
    assert len(sizes) >= 6 and [sum(sizes[:k + 1]) for k in range(4)] == cuts[:4]   # the pieces are cut where the test put the runs
    _check_child(got, buf, starts)
    base = {t[0]: t[3] for t in got["table"]}
    assert all(t[3] == base[t[0]] for t in got["table"]) and base[cuts[0]] > 0


def test_tally_beside_segments(env):
    M = env.M
    buf, starts = env.shapes()["lines_1025"]
    text = buf.tobytes()
    plain, both = M.Scanner(env.db), M.Scanner(env.db)
    try:
        for s in (plain, both):
            s.set_tally(True)
        plain.scan(text).close()
        both.set_segments(starts)
        r = both.scan(text)
        check(r, buf, starts, False, "tally", len(env.expected(buf, starts)))
        r.close()
        a, b = plain.tally(), both.tally()
        assert list(a) == list(b) and (a.distinct, a.matches) == (b.distinct, b.matches) and a.matches > 600
    finally:
        plain.close(); both.close()


def test_empty_batch_with_a_table_through_the_multi_scanner(env):
    """a batch of no bytes that carries a table is scanned like any other: its result has the table"""
    keep = ctypes.create_string_buffer(1)
    env.ms.submit_segments_ptr(ctypes.addressof(keep), 0, [0, 0])
    b = env.ms.next(want_hits=True)
    assert b["n_hits"] == 0 and b["segment_of"] == []
    assert [tuple(s.values()) for s in b["segments"]] == [(0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)]
