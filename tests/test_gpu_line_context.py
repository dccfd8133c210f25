"""GPU: line context (line index, line start, line end of every hit; distinct lines with a hit) through every scan entry, against a
numpy model written from the definitions:

    nl          = flatnonzero(buf == '\\n')
    line        = searchsorted(nl, start, "left")        number of '\\n' in buf[0, start)
    line_start  = 0 if line == 0 else nl[line - 1] + 1
    line_end    = nl[line] if line < len(nl) else len(buf)
    lines_with_matches = len(unique(line))

The logs are blanks with a handful of indicators and newlines placed where the kernels change path: LINE_TILE is the tile of the '\\n'
count array, LINE_SCAN_CHUNK tiles are the span of one workgroup of its prefix sum. Every log goes through every entry, and the hits,
ids and counters of every scan must equal those of the same scan with line context off."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
IP, DOM = b"10.1.2.3", b"evil.example.com"


def _M():
    import matchy_amd as M
    return M


def _blob(ip_only=False):
    M = _M()
    b = M.DatabaseBuilder(build_epoch=1)
    b.add_entry("10.1.2.0/24", {"k": "net"})
    b.add_entry("192.0.2.7", {"k": "host"})
    if not ip_only:
        b.add_entry("evil.example.com", {"k": "dom"})
        b.add_entry("bad.example.org", {"k": "dom2"})
    blob = b.build()
    b.close()
    return blob


def make_log(length, tokens=(), newlines=(), fill=32):
    """`length` blanks, '\\n' at `newlines`, then the tokens (pos, bytes) — each with a blank in front unless a '\\n' or the start is there, and a
    blank behind unless a '\\n' or the end is there — so that a hit starts exactly at pos."""
    buf = np.full(length, fill, dtype=np.uint8)
    nl = np.asarray(list(newlines), dtype=np.int64)
    if len(nl):
        buf[nl] = 10
    for pos, tok in tokens:
        assert 0 <= pos and pos + len(tok) <= length, (pos, length)
        if pos and buf[pos - 1] != 10:
            buf[pos - 1] = 32
        buf[pos:pos + len(tok)] = np.frombuffer(tok, dtype=np.uint8)
        if pos + len(tok) < length and buf[pos + len(tok)] != 10:
            buf[pos + len(tok)] = 32
    return buf


def model(buf, starts):
    nl = np.flatnonzero(buf == 10)
    starts = np.asarray(starts, dtype=np.int64)
    line = np.searchsorted(nl, starts, "left")
    ls = np.where(line == 0, 0, nl[np.maximum(line, 1) - 1] + 1) if len(nl) else np.zeros_like(starts)
    le = np.where(line < len(nl), nl[np.minimum(line, max(len(nl) - 1, 0))], len(buf)) if len(nl) else np.full_like(starts, len(buf))
    return np.stack([line, ls, le], axis=1).astype(np.int64)


def logs():
    M = _M()
    T, C = M.LINE_TILE, M.LINE_SCAN_CHUNK
    out = {}
    # shorter than a tile, not a multiple of 16: hit at offset 0 (its line starts at byte 0), hit in an unterminated last line
    out["short"] = make_log(100, [(0, IP), (60, DOM)], [50])
    out["no_newline"] = make_log(333, [(0, DOM), (200, IP)])
    out["one_hit_at_end"] = make_log(41, [(33, IP)], [3])
    for L in (T - 1, T, T + 1, 2 * T + 5):
        out[f"len_{L}"] = make_log(L, [(0, IP), (20, DOM), (L - 8, IP)], [17, L - 10])
    out["len_T_newline_last"] = make_log(T, [(0, IP), (T - 30, DOM)], [T - 1])
    # '\n' as the last byte of a tile with a hit on the first byte of the next; '\n' as the first byte of a tile with a hit right behind;
    # a hit on the first byte of a tile whose line began earlier
    out["tile_edges"] = make_log(4 * T + 7, [(5, IP), (T, IP), (2 * T + 1, DOM), (3 * T, IP), (4 * T - 4, IP)], [T - 1, 2 * T, 3 * T - 100])
    # a tile that is all '\n', then a hit
    out["newline_tile"] = make_log(3 * T + 40, [(5, IP), (2 * T, DOM), (2 * T + 20, IP)], range(T, 2 * T))
    out["empty_lines"] = make_log(100 + 5000 + 60, [(10, IP), (5100, DOM), (5130, IP)], range(100, 5100))
    # one line of 600 KiB with a hit in its middle, a short line, and a line of 300 KiB that runs to the end unterminated
    a, b = 1001 + 600 * 1024, 1001 + 600 * 1024 + 80
    out["long_lines"] = make_log(b + 300 * 1024 + 11, [(10, IP), (1001 + 300 * 1024 + 3, DOM), (a + 10, IP), (b + 150 * 1024 + 5, IP), (b + 300 * 1024, IP)],
                                 [1000, a, b])
    line = b"GET /x 10.1.2.3 evil.example.com ok\r\n"
    out["crlf"] = np.frombuffer(line * 50 + b"tail 10.1.2.3\r", dtype=np.uint8).copy()
    # the prefix sum with more than two workgroups: hits in the first and the last tile and on both sides of every workgroup boundary
    L = 2 * C * T + T + 123
    toks = [(0, IP), (40, DOM), (L - 8, IP), (L - T + 3, DOM)]
    for k in (1, 2):
        e = k * C * T
        toks += [(e - 9, IP), (e, DOM), (e + 30, IP), (e - T - 20, DOM), (e + T + 1, IP)]
    toks += [(p, IP if i % 3 else DOM) for i, p in enumerate(range(7001, L - 4096, 65521))]
    out["multi_chunk"] = make_log(L, toks, list(range(90, L, 97)) + [C * T - 1, 2 * C * T])
    # several hits in one line, hits in adjacent lines; every hit in the same line; every hit in a line of its own
    out["same_line"] = make_log(200 * 24 + 50, [(30 + 24 * i, IP if i % 2 else DOM) for i in range(200)], [7, 200 * 24 + 40])
    out["own_lines"] = make_log(300 * 40, [(40 * i + 4, IP) for i in range(300)] + [(40 * i + 18, DOM) for i in range(0, 300, 7)], range(39, 300 * 40, 40))
    return out


def dense_log(n_hits):
    return make_log(n_hits * 16 + 5, [(16 * i, IP) for i in range(n_hits)], range(15, n_hits * 16, 48))


# ---------------------------------------------------------------------------------------------------------------- reading results
REC = np.dtype([("start", "<u4"), ("len_type", "<u4"), ("value", "<u4"), ("kind", "u1"), ("prefix_len", "u1"), ("n_ids", "<u2")])
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    return _hip


def _array(ptr, n, dtype, device=False):
    """n records of `dtype` at address ptr (host, or device memory: copied back)"""
    nbytes = n * np.dtype(dtype).itemsize
    if not ptr or not n:
        return np.zeros(0, dtype=dtype)
    if device:
        host = (ctypes.c_uint8 * nbytes)()
        assert hip().hipMemcpy(host, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
        return np.frombuffer(bytes(host), dtype=dtype).copy()
    return np.frombuffer(ctypes.string_at(ptr, nbytes), dtype=dtype).copy()


def read(res):
    """(starts, line records [n, 3], raw 16-byte records, lines_with_matches) of a result; compact records first, like hits()"""
    raw, dev = res._raw, res.on_device
    addr = lambda p: ctypes.cast(p, ctypes.c_void_p).value or 0
    recs = _array(addr(raw.hits), raw.n_hits if raw.hits else 0, REC, dev)
    c4_starts = _array(addr(raw.ip4_hits), 2 * raw.n_ip4_hits if raw.ip4_hits else 0, np.dtype("<u4")).reshape(-1, 2)[:, 0]
    lines = _array(res.lines_ptr, len(recs) * 4, np.dtype("<u4"), dev).reshape(-1, 4)
    c4_lines = _array(res.ip4_lines_ptr, len(c4_starts) * 4, np.dtype("<u4")).reshape(-1, 4)
    starts = np.concatenate([c4_starts, recs["start"]]).astype(np.int64)
    both = np.concatenate([c4_lines, lines]) if len(c4_lines) or len(lines) else np.zeros((0, 4), "<u4")
    return starts, both, recs, res.lines_with_matches


def check_lines(res, buf, what, base=0, line_base=0):
    starts, lines, recs, lwm = read(res)
    assert res.has_lines, what
    assert len(lines) == len(starts), (what, len(lines), len(starts))
    assert (lines[:, 3] == 0).all(), what
    want = model(buf, starts)
    got = lines[:, :3].astype(np.int64)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, "first wrong record", int(starts[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist(), len(bad))
    assert lwm == len(np.unique(want[:, 0])), (what, lwm)
    return starts, recs


def snapshot(res):
    """what same_matches compares, copied out of a result: the arrays of fetch modes 0 / 1 / 1|8 / 4 are borrowed from the scanner and
    belong to its NEXT scan as soon as that runs"""
    snap = dict(counters=(res.lines, res.candidates, res.n_hits, res.n_ip4_hits), has_lines=res.has_lines, hits=None, recs=None)
    if res.on_device or not res._raw.hits and not res._raw.ip4_hits:
        return snap
    if res.n_hits <= 400:
        snap["hits"] = res.hits()
    else:
        snap["recs"] = read_recs(res)
    return snap


def same_matches(res_on, off, what, ordered):
    """hits, ids and counters of a scan with line context equal those of the same scan without (`off`: its snapshot)"""
    on = snapshot(res_on)
    assert on["counters"] == off["counters"], what
    assert on["has_lines"] and not off["has_lines"], what
    assert (on["hits"] is None) == (off["hits"] is None) and (on["recs"] is None) == (off["recs"] is None), what
    if on["hits"] is not None:
        key = lambda h: (h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]))
        a, b = on["hits"], off["hits"]
        assert (a == b) if ordered else (sorted(a, key=key) == sorted(b, key=key)), what
    if on["recs"] is not None:
        a, b = on["recs"], off["recs"]
        assert np.array_equal(a, b) if ordered else np.array_equal(np.sort(a, order=["start", "len_type"]), np.sort(b, order=["start", "len_type"])), what


def read_recs(res):
    raw = res._raw
    return _array(ctypes.cast(raw.hits, ctypes.c_void_p).value or 0, raw.n_hits if raw.hits else 0, REC, False)[["start", "len_type", "kind", "prefix_len", "n_ids"]]


class Env:
    """databases and scanners shared by the cases of this module"""

    def __init__(self):
        M = _M()
        self.M = M
        self.db, self.db4 = M.Database(_blob()), M.Database(_blob(ip_only=True))
        self.sc, self.sc4 = M.Scanner(self.db), M.Scanner(self.db4)
        self.ms = M.MultiScanner(self.db, devices=(0, 0))

    def close(self):
        for x in (self.ms, self.sc, self.sc4, self.db, self.db4):
            x.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def all_logs():
    return logs()


def on_device(buf):
    n = len(buf)
    dptr = ctypes.c_void_p()
    assert hip().hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(n + 64)) == 0
    assert hip().hipMemcpy(dptr, buf.tobytes(), ctypes.c_size_t(n), 1) == 0
    return dptr


def both(sc, run, what, ordered):
    """run() with line context off, then on: the result of the scan with it — the scanner's last scan, so its borrowed arrays are still
    its own — after comparing its match set with the one of the scan without"""
    sc.set_line_context(False)
    assert not getattr(sc, "line_context", bool)()
    off = run()
    assert not off.has_lines and off.lines_with_matches is None, what
    assert _M().lib().matchy_scan_result_lines(ctypes.byref(off._raw), None, None, None) == -5, what   # MATCHY_ERROR_INVALID_PARAM
    snap = snapshot(off)
    off.close()
    sc.set_line_context(True)
    assert getattr(sc, "line_context", lambda: True)()
    try:
        on = run()
    finally:
        sc.set_line_context(False)
    same_matches(on, snap, what, ordered)
    return on


def through_every_entry(env, buf, name, slices=False, multi_batch=0):
    text = buf.tobytes()
    sc, sc4, M = env.sc, env.sc4, env.M
    # host buffer
    on = both(sc, lambda: sc.scan(text), (name, "scan"), True)
    check_lines(on, buf, (name, "scan"))
    n_expected, want_lwm = on.n_hits, on.lines_with_matches
    assert n_expected > 0, name
    on.close()
    dptr = on_device(buf)
    try:
        for mode in (0, 1, 3, 4):
            what = (name, "scan_device", mode)
            on = both(sc, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=mode), what, mode == 3)
            if mode == 0:   # counters only: no records cross the bus, the distinct-line count still does
                assert on.has_lines and on.lines_with_matches == want_lwm and on.lines_ptr == 0, what
            else:
                assert on.on_device == (mode == 4), what
                check_lines(on, buf, what)
            assert on.n_hits == n_expected, what
            on.close()

        def submitted():
            sc.submit_device(dptr.value, len(text), fetch_mode=1)
            return sc.wait()
        on = both(sc, submitted, (name, "submit/wait"), False)
        check_lines(on, buf, (name, "submit/wait"))
        on.close()
        # the setting is read at submit
        sc.set_line_context(True)
        sc.submit_device(dptr.value, len(text), fetch_mode=1)
        sc.set_line_context(False)
        r = sc.wait()
        check_lines(r, buf, (name, "submit with, wait without"))
        r.close()
        # compact IPv4 records: a second line array parallel to ip4_hits
        on = both(sc4, lambda: sc4.scan_device(dptr.value, len(text), fetch_mode=9), (name, "compact"), False)
        assert on.n_ip4_hits > 0 and on.n_ip4_hits == on.n_hits, (name, "compact")
        check_lines(on, buf, (name, "compact"))
        on.close()
        if slices:
            for mode in (3, 9):
                s = sc4 if mode == 9 else sc
                s.set_slices(3)
                on = both(s, lambda: s.scan_device(dptr.value, len(text), fetch_mode=mode), (name, "slices", mode), mode == 3)
                assert s.last_slices() == 3
                s.set_slices(0)
                check_lines(on, buf, (name, "slices", mode))
                on.close()
    finally:
        sc.set_slices(0); sc4.set_slices(0)
        hip().hipFree(dptr)
    # all workers of a multi-scanner, merged: absolute values like scan()
    ms = env.ms
    bb = multi_batch or max(64, len(text) // 5)
    on = both(ms, lambda: ms.scan(text, batch_bytes=bb), (name, "multi scan"), True)
    check_lines(on, buf, (name, "multi scan"))
    assert on.n_hits == n_expected
    on.close()
    # ... and batch by batch: values relative to the batch
    ms.set_line_context(True)
    keep = ctypes.create_string_buffer(text, len(text))
    pos, total, lwm = 0, 0, 0
    while pos < len(text):
        end = min(pos + bb, len(text))
        if end < len(text):
            cut = text.rfind(b"\n", pos, end)
            end = cut + 1 if cut >= 0 else (text.find(b"\n", end) + 1 or len(text))
        ms.submit_ptr(ctypes.addressof(keep) + pos, end - pos)
        b = ms.next(want_hits=True)
        piece = buf[pos:end]
        starts = [h["start"] for h in b["hits"]]
        want = model(piece, starts)
        assert [list(x) for x in b["line_records"]] == want.tolist(), (name, "multi batch", pos)
        assert b["lines_with_matches"] == len(np.unique(want[:, 0])), (name, "multi batch", pos)
        total += len(starts); lwm += b["lines_with_matches"]
        pos = end
    ms.set_line_context(False)
    assert total == n_expected and lwm == want_lwm, (name, "multi batches")


SMALL = ["short", "no_newline", "one_hit_at_end", "len_T_newline_last", "tile_edges", "newline_tile", "empty_lines", "crlf", "same_line", "own_lines"]


@pytest.mark.parametrize("name", SMALL)
def test_small_logs_through_every_entry(env, all_logs, name):
    through_every_entry(env, all_logs[name], name)


def test_lengths_around_one_tile(env, all_logs):
    T = env.M.LINE_TILE
    for L in (T - 1, T, T + 1, 2 * T + 5):
        through_every_entry(env, all_logs[f"len_{L}"], f"len_{L}")


def test_lines_of_hundreds_of_tiles_without_a_newline(env, all_logs):
    through_every_entry(env, all_logs["long_lines"], "long_lines", slices=True, multi_batch=200 * 1024)


def test_prefix_sum_over_more_than_two_workgroups_and_slices(env, all_logs):
    through_every_entry(env, all_logs["multi_chunk"], "multi_chunk", slices=True, multi_batch=700 * 1024)


def test_line_array_of_a_smaller_scan_after_a_larger_one(env):
    M = env.M
    small, large = dense_log(3000), dense_log(7000)
    small[16 * 1500 + 15] = 10   # the two logs do not share their newline positions everywhere
    fresh = M.Scanner(env.db)
    used = M.Scanner(env.db)
    try:
        for s in (fresh, used):
            s.set_line_context(True)
        r = used.scan(large.tobytes())
        assert r.n_hits == 7000
        check_lines(r, large, "large")
        r.close()
        d_small = on_device(small)
        d_large = on_device(large)
        try:
            for mode in (1, 3, 4):
                r = used.scan_device(d_large.value, len(large), fetch_mode=mode)
                check_lines(r, large, ("large", mode))
                r.close()
                a = fresh.scan_device(d_small.value, len(small), fetch_mode=mode)
                b = used.scan_device(d_small.value, len(small), fetch_mode=mode)
                assert a.n_hits == b.n_hits == 3000
                sa, _ = check_lines(a, small, ("small on a fresh scanner", mode))
                sb, _ = check_lines(b, small, ("small after large", mode))
                assert a.lines_with_matches == b.lines_with_matches
                a.close(); b.close()
        finally:
            hip().hipFree(d_small); hip().hipFree(d_large)
    finally:
        fresh.close(); used.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_line_context as T
env = T.Env()
buf = T.logs()["multi_chunk"]
text = buf.tobytes()
on = T.both(env.sc, lambda: env.sc.scan(text), "pieces", True)
T.check_lines(on, buf, "pieces")
print("pieces ok", on.n_hits, on.lines_with_matches)
"""


def test_host_pieces_of_a_few_hundred_kib():
    """scan() cuts its input into pieces at newlines; with MATCHY_AMD_HOST_PIECE_BYTES the pieces are small enough that a log of a few
    MiB has more than ten of them: line numbers continue across the pieces, positions are absolute, the distinct lines add up"""
    env = dict(os.environ, MATCHY_AMD_HOST_PIECE_BYTES=str(300 * 1024), MATCHY_AMD_TRACE="1")
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "pieces ok" in p.stdout
    assert p.stderr.count("scan_host piece") >= 2 * 10   # two scans of a log of more than 4 MiB
