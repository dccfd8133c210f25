"""GPU: rendered records — the NDJSON of a scan written on the GPU (Scanner.set_render, ScanResult.rendered_ndjson) — through the scan
entries that render, every fetch mode and every flag.

The oracle is the host renderer on the same result: for a host-resident result scanned with the renderer armed, rendered_ndjson()
must equal ndjson_text / ndjson_lines_text / ndjson_segments_text of that result and its text, byte for byte. A device-resident
result (fetch mode 4) has no host renderer; its block is copied back here and compared, as a set of lines, with the host rendering
of the same scan in canonical order."""
import ctypes
import gzip

import pytest

import render_cases as R
from test_gpu_line_context import hip, on_device

pytestmark = pytest.mark.gpu

NONE, NUMBERS, INPUT = 0, 1, 3   # MATCHY_RENDER_* as the tests arm them (INPUT_LINE with the LINE_NUMBERS it implies)


def _M():
    import matchy_amd as M
    return M


class Env:
    def __init__(self):
        M = _M()
        self.M = M
        self.db = M.Database(R.built_db(M))
        self.sc = M.Scanner(self.db, profile=True)
        self.db24, self.dbv6 = M.Database(R.handmade("handmade_24.mxy")), M.Database(R.handmade("handmade_v6.mxy"))
        self.sc24, self.scv6 = M.Scanner(self.db24), M.Scanner(self.dbv6)

    def close(self):
        for x in (self.sc, self.sc24, self.scv6, self.db, self.db24, self.dbv6):
            x.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.fixture(scope="module")
def log():
    text = R.mixed_log()
    dptr = on_device(R.as_array(text))
    yield text, dptr
    hip().hipFree(dptr)


def host_text(res, text, flags, source="-", line_base=0):
    if flags == NONE:
        return res.ndjson_text(text, source=source)
    return res.ndjson_lines_text(text, source=source, line_base=line_base, with_input_line=flags == INPUT)


def armed(sc, flags, run, **kw):
    sc.set_line_context(flags != NONE)
    sc.set_render(flags=flags, **kw)
    return run()


def device_block(res):
    addr, n = res.rendered_ndjson()
    host = (ctypes.c_uint8 * max(n, 1))()
    if n:
        assert hip().hipMemcpy(host, ctypes.c_void_p(addr), ctypes.c_size_t(n), 2) == 0
    return bytes(host)[:n]


# ---------------------------------------------------------------------------------------------------------------- scan_device
@pytest.mark.parametrize("flags", [NONE, NUMBERS, INPUT])
@pytest.mark.parametrize("mode", [1, 9, 3])
def test_scan_device_equals_the_host_renderer(env, log, mode, flags):
    text, dptr = log
    res = armed(env.sc, flags, lambda: env.sc.scan_device(dptr.value, len(text), fetch_mode=mode), source='a "b".log', line_base=(1 << 33) + 5)
    assert res.n_hits > 300 and (mode != 9 or res.n_ip4_hits > 0)
    got = res.rendered_ndjson()
    want = host_text(res, text, flags, source='a "b".log', line_base=(1 << 33) + 5)
    assert got.count(b"\n") == res.n_hits
    assert got == want, next((i, got[max(0, i - 80):i + 40], want[max(0, i - 80):i + 40]) for i, (a, b) in enumerate(zip(got, want)) if a != b)
    res.close()


@pytest.mark.parametrize("flags", [NONE, INPUT])
def test_device_resident_block(env, log, flags):
    text, dptr = log
    ordered = armed(env.sc, flags, lambda: env.sc.scan_device(dptr.value, len(text), fetch_mode=3))
    want = host_text(ordered, text, flags)
    assert ordered.rendered_ndjson() == want
    ordered.close()
    res = armed(env.sc, flags, lambda: env.sc.scan_device(dptr.value, len(text), fetch_mode=4))
    assert res.on_device
    got = device_block(res)
    assert env.sc.render_counters()["copied"] == 0   # nothing of the block crossed the bus
    assert sorted(got.split(b"\n")) == sorted(want.split(b"\n"))
    res.close()


def test_counts_only_fetch_renders_nothing(env, log):
    text, dptr = log
    res = armed(env.sc, NONE, lambda: env.sc.scan_device(dptr.value, len(text), fetch_mode=0))
    with pytest.raises(ValueError):
        res.rendered_ndjson()
    res.close()
    # the parameters were consumed: the next scan is not armed
    res = env.sc.scan_device(dptr.value, len(text), fetch_mode=1)
    with pytest.raises(ValueError):
        res.rendered_ndjson()
    res.close()


def test_submit_wait_and_slices(env, log):
    text, dptr = log
    sc = env.sc

    def submitted():
        sc.submit_device(dptr.value, len(text), fetch_mode=1)
        return sc.wait()
    res = armed(sc, INPUT, submitted, source="s")
    assert res.rendered_ndjson() == host_text(res, text, INPUT, source="s")
    res.close()
    big = R.mixed_log(900)   # three slices want three segments of the streaming pass
    dbig = on_device(R.as_array(big))
    sc.set_slices(3)
    try:
        for mode in (1, 3):
            res = armed(sc, INPUT, lambda: sc.scan_device(dbig.value, len(big), fetch_mode=mode))
            assert sc.last_slices() == 3
            assert res.rendered_ndjson() == host_text(res, big, INPUT)
            res.close()
    finally:
        sc.set_slices(0)
        hip().hipFree(dbig)


@pytest.mark.parametrize("version,which", [("24", "handmade_24.mxy"), ("v6", "handmade_v6.mxy")])
def test_handmade_databases(env, version, which):
    sc = env.sc24 if version == "24" else env.scv6
    text = R.handmade_log(version)
    dptr = on_device(R.as_array(text))
    try:
        res = armed(sc, INPUT, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=3), source=which)
        assert res.n_hits > 0
        assert res.rendered_ndjson() == host_text(res, text, INPUT, source=which)
        res.close()
    finally:
        hip().hipFree(dptr)


# ---------------------------------------------------------------------------------------------------------------- scan (host buffer)
@pytest.mark.parametrize("flags", [NONE, NUMBERS, INPUT])
def test_scan_of_a_host_buffer(env, log, flags):
    text, _ = log
    res = armed(env.sc, flags, lambda: env.sc.scan(text), source="h.log", line_base=40)
    assert res.n_hits > 300 and res.rendered_ndjson() == host_text(res, text, flags, source="h.log", line_base=40)
    res.close()
    text, starts, sources, bases = R.segmented_log()
    env.sc.set_segments(starts)
    res = armed(env.sc, flags, lambda: env.sc.scan(text), sources=sources, line_bases=bases)
    assert res.rendered_ndjson() == res.ndjson_segments_text(text, sources, None if flags == NONE else bases, with_input_line=flags == INPUT)
    res.close()


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import matchy_amd as M
import render_cases as R
db = M.Database(R.built_db(M)); sc = M.Scanner(db)
sc.set_line_context(True)
text = R.mixed_log(900)   # 35 KB: three pieces of 12 KiB and a rest
sc.set_render(flags=3, source="p.log", line_base=(1 << 32) + 1)
res = sc.scan(text)
assert res.rendered_ndjson() == res.ndjson_lines_text(text, source="p.log", line_base=(1 << 32) + 1, with_input_line=True)
res.close()
parts = [R.mixed_log(200) + b"\n"] * 4 + [b"tail " + R.DOMS[0] + b"\n"]   # segments of 8 KB: they go on across the cuts
text, starts = b"".join(parts), [sum(len(q) for q in parts[:k]) for k in range(len(parts))]
sources, bases = ["s%d \"q\"" % k for k in range(len(parts))], [k << 33 for k in range(len(parts))]
sc.set_segments(starts)
sc.set_render(flags=3, sources=sources, line_bases=bases)
res = sc.scan(text)
assert res.rendered_ndjson() == res.ndjson_segments_text(text, sources, bases, with_input_line=True)
res.close(); sc.close(); db.close()
print("pieces ok")
"""


def test_scan_in_pieces_appends_the_blocks():
    """scan() cuts its input into pieces at newlines (MATCHY_AMD_HOST_PIECE_BYTES makes them small): every piece renders its records
    with the lines in front of it added to the line base, and the blocks go end to end"""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    env = dict(os.environ, MATCHY_AMD_HOST_PIECE_BYTES=str(12 * 1024), MATCHY_AMD_TRACE="1")
    p = subprocess.run([sys.executable, "-c", CHILD, str(root)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "pieces ok" in p.stdout
    assert p.stderr.count("scan_host piece") >= 3 and p.stderr.count("] render:") >= 3


# ---------------------------------------------------------------------------------------------------------------- segments, gz
@pytest.mark.parametrize("flags", [NONE, INPUT])
def test_segmented_scan(env, flags):
    text, starts, sources, bases = R.segmented_log()
    dptr = on_device(R.as_array(text))
    sc = env.sc
    try:
        for mode in (1, 3):
            sc.set_segments(starts)
            res = armed(sc, flags, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=mode), sources=sources, line_bases=bases)
            want = res.ndjson_segments_text(text, sources, None if flags == NONE else bases, with_input_line=flags == INPUT)
            assert res.n_hits > 50 and res.rendered_ndjson() == want
            res.close()
    finally:
        hip().hipFree(dptr)


def test_scan_gz_without_text(env):
    sc = env.sc
    members = [R.mixed_log(30) + b"\n", b"one " + R.IPS[0] + b"\n", R.mixed_log(20) + b"\n"]
    blobs = [gzip.compress(m) for m in members]
    sources = ["a.gz", "b \"x\".gz", "c.gz"]
    sc.set_line_context(True)
    base = sc.scan_gz(blobs, want_text=True, fetch_mode=3)
    text = base.gz_text()
    want = base.ndjson_segments_text(text, sources, [0, 0, 0], with_input_line=True)
    base.close()
    res = armed(sc, INPUT, lambda: sc.scan_gz(blobs, want_text=False, fetch_mode=3), sources=sources)
    assert res.gz_text() is None and res.n_hits > 50
    assert res.rendered_ndjson() == want
    res.close()


# ---------------------------------------------------------------------------------------------------------------- multi-device scanner
def test_multi_scanner_batches(env):
    """the parameters arm the next batch submitted and no other; the batch owns its block; plain, segmented and gz batches, on two
    workers of one device"""
    M = _M()
    ms = M.MultiScanner(env.db, devices=(0, 0))
    try:
        ms.set_line_context(True)
        a, b = R.as_array(R.mixed_log(120) + b"\n"), R.as_array(R.mixed_log(80) + b"\n")
        ms.set_render(flags=INPUT, source="m \"a\".log", line_base=(1 << 32) + 9)
        ms.submit_ptr(a.ctypes.data, len(a), tag=1)
        ms.submit_ptr(b.ctypes.data, len(b), tag=2)   # not armed
        text, starts, sources, bases = R.segmented_log()
        seg = R.as_array(text)
        ms.set_render(flags=INPUT, sources=sources, line_bases=bases)
        ms.submit_segments_ptr(seg.ctypes.data, len(seg), starts, tag=3)
        one = ms.next(want_hits=True)
        assert one["tag"] == 1 and one["n_hits"] > 100
        sc0 = M.Scanner(env.db)
        sc0.set_line_context(True)
        ref = sc0.scan(a.tobytes())
        assert one["rendered"] == ref.ndjson_lines_text(a.tobytes(), source="m \"a\".log", line_base=(1 << 32) + 9, with_input_line=True)
        ref.close()
        two = ms.next()
        assert two["tag"] == 2 and "rendered" not in two
        three = ms.next()
        sc0.set_segments(starts)
        ref = sc0.scan(text)
        assert three["tag"] == 3 and three["rendered"] == ref.ndjson_segments_text(text, sources, bases, with_input_line=True)
        ref.close()
        # a gz pack without its text
        members = [R.mixed_log(30) + b"\n", b"one " + R.IPS[0] + b"\n"]
        blobs = [gzip.compress(m) for m in members]
        packed = R.as_array(b"".join(blobs))
        table, at = [], 0
        for blob in blobs:
            table.append((at, len(blob), 0))
            at += len(blob)
        base = sc0.scan_gz(blobs, want_text=True, fetch_mode=3)
        want = base.ndjson_segments_text(base.gz_text(), ["a.gz", "b.gz"], [0, 0], with_input_line=True)
        base.close()
        sc0.close()
        ms.set_render(flags=INPUT, sources=["a.gz", "b.gz"])
        ms.submit_gz_ptr(packed.ctypes.data, len(packed), table, want_text=False, tag=4)
        four = ms.next()
        assert four["tag"] == 4 and four["text"] is None and four["rendered"] == want
    finally:
        ms.close()


# ---------------------------------------------------------------------------------------------------------------- payload table
def test_first_scan_misses_every_payload_and_the_second_none(log):
    M = _M()
    text, dptr = log
    db = M.Database(R.built_db(M))
    sc = M.Scanner(db, profile=True)
    try:
        first = armed(sc, NONE, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=3))
        a = first.rendered_ndjson()
        c = sc.render_counters()
        distinct = {h["ip_data_offset"] for h in first.hits() if h["kind"] == "ip"} | {o for h in first.hits() for o in h["offs"] if o >= 0}
        assert len(distinct) >= 7, distinct   # the log reaches (nearly) every one of the 9 payloads of the database
        assert c["rounds"] >= 1 and c["payloads_added"] == len(distinct) and c["misses"] >= len(distinct), c
        assert a == first.ndjson_text(text)
        first.close()
        second = armed(sc, NONE, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=3))
        c = sc.render_counters()
        assert (c["rounds"], c["payloads_added"], c["misses"]) == (0, 0, 0) and c["copied"] == len(a), c
        assert second.rendered_ndjson() == a
        t = sc.render_timing_ms()
        assert t["measure"] > 0 and t["write"] > 0 and t["d2h"] > 0, t
        second.close()
    finally:
        sc.close(); db.close()


def _limited(monkeypatch, name, value, log):
    """a fresh scanner that reads the limit: (status of the armed scan, text of a scan after it without the limit in its way)"""
    M = _M()
    text, dptr = log
    monkeypatch.setenv(name, value)
    db = M.Database(R.built_db(M))
    sc = M.Scanner(db)
    try:
        res = armed(sc, NONE, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=1))
        with pytest.raises(M.RenderTooLarge):
            res.rendered_ndjson()
        assert res.n_hits > 300   # the records themselves are what they were
        res.close()
        # the scanner stays usable
        res = sc.scan_device(dptr.value, len(text), fetch_mode=3)
        assert res.ndjson_text(text).count(b"\n") == res.n_hits
        res.close()
    finally:
        sc.close(); db.close()


def test_small_table_grows_and_collides(monkeypatch, log):
    """MATCHY_AMD_RENDER_PAYLOADS_SLOTS / _POOL_BYTES start table and pool tiny: a table of two slots holds one entry, so the payloads of
    the database force three growths of the slot array, probe sequences that wrap, and a pool that is regrown; the text is the host's"""
    M = _M()
    text, dptr = log
    monkeypatch.setenv("MATCHY_AMD_RENDER_PAYLOADS_SLOTS", "2")
    monkeypatch.setenv("MATCHY_AMD_RENDER_PAYLOADS_POOL_BYTES", "16")
    db = M.Database(R.built_db(M))
    sc = M.Scanner(db)
    try:
        first = armed(sc, INPUT, lambda: sc.scan_device(dptr.value, len(text), fetch_mode=3))
        c = sc.render_counters()
        assert c["payloads_added"] >= 7 and c["rehashes"] >= 3 and c["pool_regrows"] >= 1, c   # 2 -> 4 -> 8 -> 16 slots for 7 to 9 entries
        assert first.rendered_ndjson() == host_text(first, text, INPUT)
        first.close()
        # a second batch with other payloads joins a table that is already full to its half
        other = b"x 203.0.113.9 y\n" + text
        dother = on_device(R.as_array(other))
        try:
            res = armed(sc, NONE, lambda: sc.scan_device(dother.value, len(other), fetch_mode=3))
            assert res.rendered_ndjson() == host_text(res, other, NONE) and sc.render_counters()["rounds"] == 0
            res.close()
        finally:
            hip().hipFree(dother)
    finally:
        sc.close(); db.close()


def test_more_distinct_payloads_than_the_table_may_hold(monkeypatch, log):
    _limited(monkeypatch, "MATCHY_AMD_RENDER_PAYLOADS", "4", log)


def test_demand_above_the_byte_limit(monkeypatch, log):
    _limited(monkeypatch, "MATCHY_AMD_RENDER_MAX_BYTES", "64", log)


# ---------------------------------------------------------------------------------------------------------------- errors, off path
def test_parameters_that_do_not_fit_the_scan(env, log):
    M = _M()
    text, dptr = log
    sc = env.sc
    sc.set_line_context(False)
    sc.set_render(flags=INPUT)   # line flags without line context
    with pytest.raises(RuntimeError, match="line context"):
        sc.scan_device(dptr.value, len(text), fetch_mode=1)
    sc.set_render(flags=NONE, sources=["a", "b"])   # sources for a scan without segments
    with pytest.raises(RuntimeError, match="no segments"):
        sc.scan_device(dptr.value, len(text), fetch_mode=1)
    sc.set_segments([0, 10])
    sc.set_render(flags=NONE, sources=["a", "b", "c"])   # another number of sources than segments
    with pytest.raises(RuntimeError, match="3 sources"):
        sc.scan_device(dptr.value, len(text), fetch_mode=1)
    sc.set_render(flags=INPUT)
    with pytest.raises(RuntimeError, match="line context"):   # the host entry checks the same
        sc.scan(text)
    # usable, and not armed
    res = sc.scan_device(dptr.value, len(text), fetch_mode=1)
    assert res.n_hits > 300
    assert M.lib().matchy_scan_result_ndjson(ctypes.byref(res._raw), None, None, None) == -5   # MATCHY_ERROR_INVALID_PARAM
    res.close()


def test_never_armed_nothing_changes(log):
    M = _M()
    text, dptr = log
    db = M.Database(R.built_db(M))
    plain, other = M.Scanner(db), M.Scanner(db)
    try:
        a = plain.scan_device(dptr.value, len(text), fetch_mode=3)
        want = a.ndjson_text(text)
        assert plain.render_counters() == dict(rounds=0, misses=0, payloads_added=0, copied=0, rehashes=0, pool_regrows=0)
        assert plain.render_timing_ms() == dict(measure=0.0, write=0.0, d2h=0.0)
        b = armed(other, NONE, lambda: other.scan_device(dptr.value, len(text), fetch_mode=3))
        assert a.hits() == b.hits() and b.ndjson_text(text) == want == b.rendered_ndjson()
        a.close(); b.close()
    finally:
        plain.close(); other.close(); db.close()
