"""GPU: hit lines — the distinct lines with a hit, gathered into one block on the GPU — through every scan entry and fetch mode,
against the numpy model of tests/hit_lines_cases.py (the block contract of include/matchy_amd.h).

Every log is scanned twice per entry: with line context alone (the baseline: hits, ids, counters, line records, and the NDJSON of
every renderer from the WHOLE text) and with hit lines. The second scan must deliver the same hits, ids, counters and line records, a
block that equals the model, and — with text = NULL — byte for byte the NDJSON of the baseline."""
import ctypes

import numpy as np
import pytest

import gz_cases as G
import hit_lines_cases as H
from test_gpu_line_context import _array, _blob, hip, on_device, read

pytestmark = pytest.mark.gpu


def _M():
    import matchy_amd as M
    return M


class Env:
    def __init__(self):
        M = _M()
        self.M = M
        self.db, self.db4, self.dbg = M.Database(_blob()), M.Database(_blob(ip_only=True)), M.Database(G.blob())
        self.sc, self.sc4, self.scg = M.Scanner(self.db), M.Scanner(self.db4), M.Scanner(self.dbg)

    def close(self):
        for x in (self.sc, self.sc4, self.scg, self.db, self.db4, self.dbg):
            x.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def all_logs():
    return H.logs(_M())


# ---------------------------------------------------------------------------------------------------------------- reading results
def read_block(res):
    """(text, line_off, line_no, line_of in the order of read(): compact records first) of a result with a gathered block"""
    hl = res.hit_lines()
    assert hl is not None
    n_hits = res._raw.n_hits if res._raw.hits else 0
    n_ip4 = res._raw.n_ip4_hits if res._raw.ip4_hits else 0
    if hl["on_device"]:
        u32 = np.dtype("<u4")
        text = _array(hl["text"], hl["text_len"], np.uint8, True).tobytes()
        off = _array(hl["line_off"], hl["n_lines"] + 1, u32, True)
        no = _array(hl["line_no"], hl["n_lines"], u32, True)
        of = _array(hl["line_of_hit"], n_hits, u32, True)
        of4 = np.zeros(0, u32)
    else:
        z = np.zeros(0, np.uint32)
        text, off = hl["text"], hl["line_off"]
        no = hl["line_no"] if hl["line_no"] is not None else z
        of = hl["line_of_hit"] if hl["line_of_hit"] is not None else z
        of4 = hl["line_of_ip4_hit"] if hl["line_of_ip4_hit"] is not None else z
    assert len(of) == n_hits and len(of4) == n_ip4
    return hl, text, off.astype(np.int64), no.astype(np.int64), np.concatenate([of4, of]).astype(np.int64)


def check_block(res, buf, what):
    starts, lines, _, lwm = read(res)
    hl, text, off, no, of = read_block(res)
    w_text, w_off, w_no, w_of = H.block_model(buf, starts)
    assert hl["n_lines"] == len(w_no) == lwm, (what, hl["n_lines"], len(w_no), lwm)
    assert hl["text_len"] == len(w_text) and hl["text_len"] <= len(buf) + 1, (what, hl["text_len"], len(w_text))
    assert np.array_equal(off, w_off), (what, "line_off")
    assert np.array_equal(no, w_no), (what, "line_no")
    assert np.array_equal(of, w_of), (what, "line_of")
    assert text == w_text, (what, "text", next((i for i, (a, b) in enumerate(zip(text, w_text)) if a != b), None))
    # the text of every hit through the documented expression
    for i in range(min(len(starts), 300)):
        k = of[i]
        at = off[k] + (starts[i] - int(lines[i, 1]))
        assert text[at:at + 4] == buf[starts[i]:starts[i] + 4].tobytes(), (what, i)


class Baseline:
    """what the scan with line context alone delivered, copied out (its arrays belong to the scanner's next scan), and its NDJSON from
    the whole text"""

    def __init__(self, res, text, ordered, sources=None, line_bases=None):
        self.counters = (res.lines, res.candidates, res.n_hits, res.n_ip4_hits, res.lines_with_matches)
        self.host = not res.on_device and bool(res._raw.hits or res._raw.ip4_hits)
        self.hits = self.lines = self.nd = self.ndl = self.nds = self.one = None
        if res.on_device:
            starts, lines, recs, _ = read(res)
            self.lines = (starts, lines, recs)
        if self.host:
            starts, lines, _, _ = read(res)
            self.hits, self.lines = res.hits(), (starts, lines)
            self.nd = res.ndjson_text(text)
            self.ndl = res.ndjson_lines_text(text, source="src", line_base=7, with_input_line=True)
            if sources is not None:
                self.nds = res.ndjson_segments_text(text, sources, line_bases, with_input_line=True)
            if len(self.hits) <= 400:
                self.one = res.ndjson(text, source="one")
        self.ordered = ordered


def lines_of(nd, ordered):
    rows = nd.split(b"\n")
    return rows if ordered else sorted(rows)


def same_as_baseline(on, base, what, sources=None, line_bases=None):
    assert (on.lines, on.candidates, on.n_hits, on.n_ip4_hits, on.lines_with_matches) == base.counters, what
    if on.on_device:
        starts, lines, recs, _ = read(on)
        order_a, order_b = np.argsort(starts, kind="stable"), np.argsort(base.lines[0], kind="stable")
        assert np.array_equal(starts[order_a], base.lines[0][order_b]) and np.array_equal(lines[order_a], base.lines[1][order_b]), what
        return
    if not base.host:
        return
    key = lambda h: (h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]))
    a, b = on.hits(), base.hits
    assert (a == b) if base.ordered else (sorted(a, key=key) == sorted(b, key=key)), what
    starts, lines, _, _ = read(on)
    order_a, order_b = np.argsort(starts, kind="stable"), np.argsort(base.lines[0], kind="stable")
    assert np.array_equal(lines[order_a], base.lines[1][order_b]), what
    # every renderer with text = NULL
    assert lines_of(on.ndjson_text(None), base.ordered) == lines_of(base.nd, base.ordered), (what, "to_ndjson")
    assert lines_of(on.ndjson_lines_text(None, source="src", line_base=7, with_input_line=True), base.ordered) == lines_of(base.ndl, base.ordered), (what, "to_ndjson_lines")
    if sources is not None:
        assert lines_of(on.ndjson_segments_text(None, sources, line_bases, with_input_line=True), base.ordered) == lines_of(base.nds, base.ordered), (what, "to_ndjson_segments")
    if base.one is not None:
        got = on.ndjson(None, source="one")
        assert None not in got, what
        assert got == base.one if base.ordered else sorted(got) == sorted(base.one), (what, "hit_to_json")


def pair(sc, run, text, what, ordered, sources=None, line_bases=None, prepare=None):
    """run() with line context alone, then with hit lines: the second result, compared with the first"""
    M = _M()
    sc.set_line_context(True)
    sc.set_hit_lines(False)
    assert not sc.hit_lines_enabled()
    if prepare:
        prepare()
    off = run()
    assert off.hit_lines() is None, what
    assert M.lib().matchy_scan_result_hit_lines(ctypes.byref(off._raw), ctypes.byref(M._ScanHitLines())) == -5, what   # MATCHY_ERROR_INVALID_PARAM
    if not off.on_device and (off._raw.hits or off._raw.ip4_hits) and off.n_hits:
        with pytest.raises(RuntimeError):
            off.ndjson_text(None)   # without the block a renderer still needs the text
    base = Baseline(off, text, ordered, sources, line_bases)
    off.close()
    sc.set_line_context(False)   # hit lines turn line context on by themselves
    sc.set_hit_lines(True)
    assert sc.hit_lines_enabled()
    if prepare:
        prepare()
    try:
        on = run()
    finally:
        sc.set_hit_lines(False)
    assert on.has_lines, what
    same_as_baseline(on, base, what, sources, line_bases)
    return on


def through_every_entry(env, buf, name, expect_hits=True):
    text = buf.tobytes()
    sc, sc4 = env.sc, env.sc4
    on = pair(sc, lambda: sc.scan(text), text, (name, "scan"), True)
    check_block(on, buf, (name, "scan"))
    n_expected, want_lwm = on.n_hits, on.lines_with_matches
    assert (n_expected > 0) == expect_hits, name
    on.close()
    dptr = on_device(buf)
    try:
        for mode in (0, 1, 3, 4):
            what = (name, "scan_device", mode)
            on = pair(sc, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=mode), text, what, mode == 3)
            assert on.n_hits == n_expected, what
            if mode == 0:   # counts only: the gather does not run
                hl = on.hit_lines()
                assert hl["n_lines"] == want_lwm and hl["text_len"] == 0 and hl["text"] is None, what
                assert hl["line_off"] is None and hl["line_no"] is None and hl["line_of_hit"] is None and hl["line_of_ip4_hit"] is None, what
            else:
                assert on.on_device == (mode == 4), what
                check_block(on, buf, what)
            on.close()

        def submitted():
            sc.submit_device(dptr.value, len(text), fetch_mode=1)
            return sc.wait()
        on = pair(sc, submitted, text, (name, "submit/wait"), False)
        check_block(on, buf, (name, "submit/wait"))
        on.close()
        # the setting is read at submit
        sc.set_hit_lines(True)
        sc.submit_device(dptr.value, len(text), fetch_mode=1)
        sc.set_hit_lines(False)
        r = sc.wait()
        check_block(r, buf, (name, "submit with, wait without"))
        r.close()
        # IPv4-only database, compact records: line_of_ip4_hit
        on = pair(sc4, lambda: sc4.scan_device(dptr.value, len(text), fetch_mode=9), text, (name, "compact"), False)
        if expect_hits:
            assert on.n_ip4_hits > 0 and on.n_ip4_hits == on.n_hits, (name, "compact")
        check_block(on, buf, (name, "compact"))
        on.close()
    finally:
        hip().hipFree(dptr)


NAMES = ["last_line_unterminated", "no_newline", "same_line", "numbered_lines", "crlf", "line_is_its_token", "long_line", "bad_utf8", "many_hit_lines",
         "slice_edges"]


@pytest.mark.parametrize("name", NAMES)
def test_logs_through_every_entry(env, all_logs, name):
    through_every_entry(env, all_logs[name], name)


def test_log_without_a_hit(env):
    buf = H.empty_log()
    through_every_entry(env, buf, "empty", expect_hits=False)
    env.sc.set_hit_lines(True)
    try:
        r = env.sc.scan(buf.tobytes())
        hl = r.hit_lines()
        assert hl["n_lines"] == 0 and hl["text_len"] == 0 and hl["text"] == b"" and hl["line_off"].tolist() == [0]
        assert r.ndjson_text(None) == b""
        r.close()
    finally:
        env.sc.set_hit_lines(False)


def test_numbered_lines_are_where_the_rank_step_changes_workgroup(env, all_logs):
    C = env.M.HIT_LINES_SCAN_CHUNK
    env.sc.set_hit_lines(True)
    try:
        r = env.sc.scan(all_logs["numbered_lines"].tobytes())
        assert r.hit_lines()["line_no"].tolist() == [0, 31, 32, 63, 64, 32 * C - 1, 32 * C, 32 * C + 1, 32 * C + 39]
        r.close()
    finally:
        env.sc.set_hit_lines(False)


def test_block_regrows_and_leaves_nothing_stale(env):
    """small, 50 x larger, small again on one scanner, every fetch mode that gathers: the block of the large scan does not fit the
    capacity the small one left (the copy kernel runs again), and the small scan behind it shows no byte or length of the large one"""
    M = env.M
    small, large, small2 = H.sized_log(40), H.sized_log(2000), H.sized_log(37)
    sc = M.Scanner(env.db, profile=True)
    sc.set_hit_lines(True)
    bufs = [(b, on_device(b)) for b in (small, large, small2)]
    try:
        for mode in (1, 3, 4):
            for buf, dptr in bufs:
                r = sc.scan_device(dptr.value, len(buf), fetch_mode=mode)
                assert r.n_hits > 0
                check_block(r, buf, ("regrow", mode, len(buf)))
                t = sc.hit_lines_timing_ms()
                assert t["index"] > 0 and t["copy_kernel"] > 0 and (t["d2h"] > 0) == (mode != 4), t
                r.close()
        for buf in (small, large, small2):
            r = sc.scan(buf.tobytes())
            check_block(r, buf, ("regrow", "scan", len(buf)))
            r.close()
    finally:
        for _, dptr in bufs:
            hip().hipFree(dptr)
        sc.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_hit_lines as T
env = T.Env()
buf = T.H.logs(env.M)["many_hit_lines"]
text = buf.tobytes()
on = T.pair(env.sc, lambda: env.sc.scan(text), text, "pieces", True)
T.check_block(on, buf, "pieces")
print("pieces ok", on.n_hits, on.hit_lines()["n_lines"])
"""


def test_host_pieces_append_their_blocks():
    """scan() cuts its input into pieces at newlines (MATCHY_AMD_HOST_PIECE_BYTES makes them small): the blocks of the pieces go end to
    end, line numbers and ranks continue across them"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, MATCHY_AMD_HOST_PIECE_BYTES=str(20 * 1024), MATCHY_AMD_TRACE="1")
    p = subprocess.run([sys.executable, "-c", CHILD, str(root)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "pieces ok" in p.stdout
    assert p.stderr.count("scan_host piece") >= 2 * 5 and p.stderr.count("hit lines:") >= 5


def test_segmented_scan(env):
    """a pack of small inputs: the block is that of the whole batch, and the segment renderer reads it"""
    sc = env.sc
    parts = [b"a 10.1.2.3 x\nnothing\n", b"", b"evil.example.com\n\xff 10.1.2.9 evil.example.com tail\n", b"none\n", b"last 192.0.2.7 line\n"]
    starts, pos = [], 0
    for p in parts:
        starts.append(pos)
        pos += len(p)
    text = b"".join(parts)
    buf = np.frombuffer(text, dtype=np.uint8).copy()
    sources = ["file%d.log" % i for i in range(len(parts))]
    bases = [100 * i for i in range(len(parts))]
    prepare = lambda: sc.set_segments(starts)
    on = pair(sc, lambda: sc.scan(text), text, "segments scan", True, sources, bases, prepare)
    check_block(on, buf, "segments scan")
    assert [s["hits"] for s in on.segments] == [1, 0, 3, 0, 1]
    on.close()
    dptr = on_device(buf)
    try:
        for mode in (1, 3, 4):
            on = pair(sc, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=mode), text, ("segments", mode), mode == 3, sources, bases, prepare)
            check_block(on, buf, ("segments", mode))
            on.close()
    finally:
        hip().hipFree(dptr)


def gz_pack():
    texts = [G.log(3 + i % 5, seed=i + 1, final_newline=i % 7 != 3) for i in range(40)]
    blobs = [G.gz_wrap(G.raw_deflate(t), t) for t in texts]
    blobs[17] = G.gz_wrap(G.raw_deflate(texts[17]), texts[17], crc=1)   # a corrupt member: its region holds no hit
    return texts, blobs


def test_gz_scan_without_the_inflated_text(env):
    """want_text=False with hit lines against want_text=True without: same records, and the renderers need no text"""
    sc = env.scg
    texts, blobs = gz_pack()
    sources = ["m%d.gz" % i for i in range(len(blobs))]
    bases = [0] * len(blobs)
    for mode in (1, 3):
        sc.set_hit_lines(False)
        sc.set_line_context(True)
        off = sc.scan_gz(blobs, want_text=True, fetch_mode=mode)
        status = off.gz_status()
        assert status[17] == G.STATUS.index("CRC_MISMATCH") and sum(1 for s in status if s) == 1
        text = off.gz_text()
        base = Baseline(off, text, mode == 3, sources, bases)
        off.close()
        sc.set_line_context(False)
        sc.set_hit_lines(True)
        try:
            on = sc.scan_gz(blobs, want_text=False, fetch_mode=mode)
        finally:
            sc.set_hit_lines(False)
        assert on.gz_text() is None and on.gz_text_len() == len(text) and on.gz_status() == status
        assert on.n_hits > 40
        same_as_baseline(on, base, ("gz", mode), sources, bases)
        check_block(on, np.frombuffer(text, dtype=np.uint8), ("gz", mode))
        on.close()


def test_multi_scanner_plain_and_gz(env):
    M = env.M
    buf = H.logs(M)["bad_utf8"]
    text = buf.tobytes()
    texts, blobs = gz_pack()
    sc = env.scg
    # the baselines: canonical order, rendered from the whole text
    sc.set_line_context(True)
    r = sc.scan(text)
    want_plain = r.ndjson_lines_text(text, with_input_line=True)
    n_plain = r.n_hits
    r.close()
    r = sc.scan_gz(blobs, want_text=True, fetch_mode=3)
    gz_text = r.gz_text()
    want_gz = r.ndjson_lines_text(gz_text, with_input_line=True)
    r.close()
    sc.set_line_context(False)
    assert n_plain > 0 and want_gz
    ms = M.MultiScanner(env.dbg, devices=(0,))
    try:
        ms.set_hit_lines(True)
        keep = ctypes.create_string_buffer(text, len(text))
        ms.submit_ptr(ctypes.addressof(keep), len(text))
        b = ms.next(want_hits=True)
        assert b["ndjson_lines"] == want_plain
        starts = [h["start"] for h in b["hits"]]
        w_text, w_off, w_no, w_of = H.block_model(buf, starts)
        hl = b["hit_lines"]
        assert hl["text"] == w_text and hl["line_off"].tolist() == w_off.tolist() and hl["line_no"].tolist() == w_no.tolist() and hl["line_of_hit"].tolist() == w_of.tolist()
        packed = ctypes.create_string_buffer(b"".join(blobs), sum(len(x) for x in blobs))
        members, pos = [], 0
        for x in blobs:
            members.append((pos, len(x), 0))
            pos += len(x)
        ms.submit_gz_ptr(ctypes.addressof(packed), pos, members, want_text=False)
        b = ms.next(want_hits=True)
        assert b["text"] is None and b["ndjson_lines"] == want_gz
        gbuf = np.frombuffer(gz_text, dtype=np.uint8)
        w_text, w_off, w_no, w_of = H.block_model(gbuf, [h["start"] for h in b["hits"]])
        assert b["hit_lines"]["text"] == w_text and b["hit_lines"]["line_of_hit"].tolist() == w_of.tolist()
        # off again: batches carry no block
        ms.set_hit_lines(False)
        ms.submit_ptr(ctypes.addressof(keep), len(text))
        b = ms.next(want_hits=True)
        assert "hit_lines" not in b
    finally:
        ms.close()
