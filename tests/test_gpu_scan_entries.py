"""GPU: one small text through every scan entry of the C API — matchy_scanner_scan, _scan_device, _submit_device + _wait and _scan_gz (one
deflated member) — with one segment, line context, hit lines and rendered records set, in every fetch mode. The entries share one route
from a fetch mode to a result, so for each mode the hit records, line records, segment indices, the block of hit lines and the rendered
NDJSON agree between the entries, and the rendered block equals the host renderer's text of the same result.

What the gz entry does differently, and the test pins: its batch is the member's text plus the '\\n' that seals it, so its one segment is
one byte longer; `lines` does not count that byte."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_gpu_line_context import hip, on_device

pytestmark = pytest.mark.gpu

SOURCE, LINE_BASE = 'x "1".log', 7
COUNTS, HITS, SORTED, COMPACT, DEVICE = 0, 1, 3, 1 | 8, 4
DEVICE_ENTRIES = ("scan_device", "submit_wait", "scan_gz")


def make_text():
    """200 short lines; every tenth one carries something the database lists, one of them two things, and the lines around the
    IPv6 hit hold '"', a backslash and ill-formed UTF-8"""
    hit = [b"client 10.1.2.%d ok", b"from 2001:db8::%x \"q\\\" \xff\xe0\xa0", b"GET http://evil.example.com/%d", b"ref cdn%d.bad.example.org end"]
    out = []
    for i in range(200):
        if i % 10 == 3:
            out.append(hit[(i // 10) % 4] % (i + 1))
        elif i == 77:
            out.append(b"two 192.0.2.7 and evil.example.com here")
        else:
            out.append(b"line %d of nothing 203.0.113.%d www.example.net" % (i, i))
    return b"\n".join(out) + b"\n"


def snapshot(res, text, entry, mode):
    """everything a result says, as plain Python data (borrowed results point into the scanner's pinned blocks: read before the next scan)"""
    s = dict(n_hits=res.n_hits, n_ip4=res.n_ip4_hits, lines=res.lines, candidates=res.candidates, bytes=res.bytes, lines_with_matches=res.lines_with_matches,
             segments=res.segments, on_device=res.on_device)
    hl = res.hit_lines()
    s["hl_n_lines"] = hl["n_lines"]
    if mode == DEVICE:
        return s
    s["block"] = None if hl["line_off"] is None else (hl["text"], hl["line_off"].tolist(), hl["line_no"].tolist())
    if mode == COUNTS:
        with pytest.raises(ValueError):   # a counts-only fetch renders nothing
            res.rendered_ndjson()
        assert res.hits() == [] and res.line_records == [] and res.segment_of == []
        return s
    hits = res.hits()   # the compact records first, then the 16-byte ones
    lines = res.ip4_lines + res.line_records
    segs = res.segment_of_ip4 + res.segment_of
    of = ([] if hl["line_of_ip4_hit"] is None else hl["line_of_ip4_hit"].tolist()) + hl["line_of_hit"].tolist()
    assert len(hits) == len(lines) == len(segs) == len(of) == res.n_hits
    block_line = [hl["text"][hl["line_off"][k]:hl["line_off"][k + 1]] for k in of]
    s["records"] = [(h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]), l, g, b)
                    for h, l, g, b in zip(hits, lines, segs, block_line)]
    s["rendered"] = res.rendered_ndjson()
    # the same result through the host renderer: from the batch, and from its block of hit lines
    s["host"] = res.ndjson_lines_text(text, source=SOURCE, line_base=LINE_BASE, with_input_line=True)
    s["host_from_block"] = res.ndjson_lines_text(None, source=SOURCE, line_base=LINE_BASE, with_input_line=True)
    s["host_plain"] = res.ndjson_text(text, source=SOURCE)
    s["single"] = res.ndjson(text, source=SOURCE)
    return s


@pytest.fixture(scope="module")
def runs():
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1)
    for key, data in (("10.1.2.0/24", {"k": "net"}), ("192.0.2.7", {"k": "host"}), ("2001:db8::/32", {"k": "six", "n": [1, 2]}),
                      ("evil.example.com", {"k": "dom"}), ("*.bad.example.org", {"k": "glob"}), ("*.example.com", {"k": "glob2"})):
        b.add_entry(key, data)
    blob = b.build()
    b.close()
    text = make_text()
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    gz = c.compress(text) + c.flush()
    dptr = on_device(np.frombuffer(text, dtype=np.uint8))
    db = M.Database(blob)
    sc = M.Scanner(db)
    sc.set_line_context(True)
    sc.set_hit_lines(True)

    def arm(segments):
        if segments:
            sc.set_segments([0])
        sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)

    out = {}
    for mode in (COUNTS, HITS, SORTED, COMPACT, DEVICE):
        for entry in ("scan", "scan_device", "submit_wait", "scan_gz"):
            if entry == "scan" and mode != SORTED:
                continue   # matchy_scanner_scan has no fetch mode: its result is the sorted, owned one
            arm(entry != "scan_gz")   # a gz scan brings its own table: one segment per member
            if entry == "scan":
                res = sc.scan(text)
            elif entry == "scan_device":
                res = sc.scan_device(dptr.value, len(text), fetch_mode=mode)
            elif entry == "submit_wait":
                sc.submit_device(dptr.value, len(text), fetch_mode=mode)
                res = sc.wait()
            else:
                res = sc.scan_gz([gz], fetch_mode=mode)
                assert res.gz_status() == [0]
            out[entry, mode] = snapshot(res, text, entry, mode)
            if mode == DEVICE:
                out[entry, mode]["refusals"] = refusals(M, sc, res, text)
            res.close()
    sc.close()
    db.close()
    hip().hipFree(dptr)
    return dict(text=text, runs=out)


def refusals(M, sc, res, text):
    """what the host readers say to a result whose records are in device memory"""
    said = []
    for call in (lambda: res.ndjson_text(text, source=SOURCE), lambda: res.ndjson_lines_text(text, source=SOURCE, with_input_line=True)):
        with pytest.raises(RuntimeError) as e:
            call()
        said.append(str(e.value))
    assert not M.lib().matchy_scan_hit_to_json(sc._h, C.byref(res._raw), 0, text, b"-")
    said.append(M.last_error())
    return said


def same_but_gz_seal(a, b, text):
    """two snapshots' counters and segment tables; the gz batch is one '\\n' longer than the text"""
    for k in ("n_hits", "n_ip4", "lines", "candidates", "bytes", "lines_with_matches", "hl_n_lines", "on_device"):
        assert a[k] == b[k], k
    sa, sb = [dict(s) for s in a["segments"]], [dict(s) for s in b["segments"]]
    assert len(sa) == len(sb) == 1
    assert (sa[0].pop("len"), sb[0].pop("len")) == (len(text), len(text) + 1)
    assert (sa[0].pop("lines"), sb[0].pop("lines")) == (text.count(b"\n"), text.count(b"\n") + 1)
    assert sa == sb


@pytest.mark.parametrize("mode", [COUNTS, HITS, SORTED, COMPACT], ids=["counts", "hits", "sorted", "compact"])
def test_entries_agree(runs, mode):
    text, r = runs["text"], runs["runs"]
    first = r["scan_device", mode]
    assert (first["n_hits"], first["lines"], first["bytes"], first["lines_with_matches"], first["on_device"]) == (22, 200, len(text), 21, False)
    assert first["segments"] == [dict(start=0, len=len(text), hits=22, line_base=0, lines=200, lines_with_matches=21)]
    entries = [e for e in ("scan", "scan_device", "submit_wait", "scan_gz") if (e, mode) in r]
    # records and rendered lines: the order of the device's records may differ between two scans of an unsorted fetch
    key = (lambda x: x) if mode == SORTED else sorted
    for entry in entries:
        other = r[entry, mode]
        if entry == "scan_gz":
            same_but_gz_seal(first, other, text)
        else:
            for k in ("n_hits", "lines", "candidates", "bytes", "lines_with_matches", "hl_n_lines", "segments", "on_device"):
                assert first[k] == other[k], (entry, k)
        assert first["block"] == other["block"], entry   # the block depends on the batch and the set of hits alone
        if mode == COUNTS:
            assert other["block"] is None and other["hl_n_lines"] == 21
            continue
        assert key(first["records"]) == key(other["records"]), entry
        assert key(first["rendered"].split(b"\n")) == key(other["rendered"].split(b"\n")), entry
        # the rendered block of a result is the host renderer's text of the same result, from the batch and from the block
        assert other["rendered"] == other["host"] == other["host_from_block"], entry
        assert other["rendered"].count(b"\n") == 22 and b'"input_line":"from 2001:db8::' in other["rendered"] and b'"source":"x \\"1\\".log"' in other["rendered"]
        assert "".join(x + "\n" for x in other["single"]).encode() == other["host_plain"], entry
        assert len(other["records"]) == 22 and {x[3] for x in other["records"]} == {"ip", "pattern"}
        assert (other["n_ip4"] > 0) == (mode == COMPACT), entry


def test_sorted_results_equal_the_host_entry(runs):
    r = runs["runs"]
    for entry in ("scan_device", "submit_wait", "scan_gz"):
        for k in ("records", "rendered", "host", "host_plain", "single", "block"):
            assert r["scan", SORTED][k] == r[entry, SORTED][k], (entry, k)
    starts = [x[0] for x in r["scan", SORTED]["records"]]
    assert starts == sorted(starts)


def test_device_fetch(runs):
    text, r = runs["text"], runs["runs"]
    first = r["scan_device", DEVICE]
    assert first["on_device"] and first["n_hits"] == 22
    same_but_gz_seal(first, r["scan_gz", DEVICE], text)
    for entry in DEVICE_ENTRIES:
        s = r[entry, DEVICE]
        if entry != "scan_gz":
            assert {k: v for k, v in s.items() if k != "refusals"} == {k: v for k, v in first.items() if k != "refusals"}
        assert s["refusals"] == [
            "matchy_scan_result_to_ndjson failed (-5): matchy_scan_result_to_ndjson: the records of this result are in device memory (MATCHY_SCAN_FETCH_DEVICE)",
            "matchy_scan_result_to_ndjson_lines failed (-5): matchy_scan_result_to_ndjson: the records of this result are in device memory (MATCHY_SCAN_FETCH_DEVICE)",
            "matchy_scan_hit_to_json: the records of this result are in device memory (MATCHY_SCAN_FETCH_DEVICE)"], entry
