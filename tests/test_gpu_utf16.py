"""GPU: UTF-16 inputs (matchy_scanner_scan_utf16, csrc/utf16.hip). Expected bytes come from the pure-Python reference of
tests/utf16_cases.py, which tests/test_utf16_host.py holds against the interpreter's codec and against the CPU driver of the same rules;
expected records come from the existing path: matchy_scanner_scan of the UTF-8 text. Shapes follow matchy_amd_utf16_geometry."""
import ctypes as C

import numpy as np
import pytest

import gz_cases as G
import utf16_cases as U
from test_gpu_line_context import hip, on_device, read

pytestmark = pytest.mark.gpu

COUNTS, HITS, SORTED, COMPACT, DEVICE = 0, 1, 3, 1 | 8, 4
SOURCE, LINE_BASE = 'w "16".log', 3
INVALID = -5
A3 = "€"   # a unit of three bytes


class Env:
    def __init__(self):
        import matchy_amd as M
        self.M = M
        self.db = M.Database(G.blob())
        self.sc = M.Scanner(self.db)      # UTF-16 scans
        self.ref = M.Scanner(self.db)     # the reference: scans of the UTF-8 text
        self.T, self.C = M.utf16_geometry()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.sc.close(); e.ref.close(); e.db.close()


def transcode(env, data, order, fetch_mode=COUNTS):
    """(text, code units, U+FFFD) of one call with want_text, the result's own figures checked against each other"""
    r = env.sc.scan_utf16(data, order, want_text=True, fetch_mode=fetch_mode)
    u = r.utf16()
    assert u is not None and u["text"] is not None and u["text_len"] == len(u["text"]) == r.bytes
    assert r.lines == u["text"].count(b"\n")
    r.close()
    return u["text"], u["code_units"], u["replaced"]


def check(env, data, order, want, what):
    text, units, replaced = transcode(env, data, order)
    if text != want[0]:   # name the first difference instead of printing megabytes
        n = min(len(text), len(want[0]))
        at = next((i for i in range(n) if text[i] != want[0][i]), n)
        raise AssertionError(f"{what}: text differs at byte {at} (lengths {len(text)}, {len(want[0])}): {text[max(at - 8, 0):at + 8]!r} for {want[0][max(at - 8, 0):at + 8]!r}")
    assert (units, replaced) == want[1:], what


def test_geometry(env):
    assert env.T == 1024 and env.C >= 2 and env.T % 16 == 0


def test_every_case_in_its_own_call(env):
    """(a): every named and generated case, both byte orders, each its own call; then the even-length cases of a byte order end to end
    as one input"""
    inputs = U.all_inputs()
    for name, order, data in inputs:
        check(env, data, order, U.reference(data, order), name)
    for order in (U.LE, U.BE):
        joined = b"".join(d for _, o, d in inputs if o == order and len(d) % 2 == 0)
        assert len(joined) > 8 * env.T
        check(env, joined, order, U.reference(joined, order), f"all even cases of {U.CODEC[order]} end to end")
        check(env, joined + b"\xd8", order, U.reference(joined + b"\xd8", order), f"all even cases of {U.CODEC[order]} end to end, odd length")


def build(pieces, order, odd=None):
    """pieces: [(units, utf-8 bytes, U+FFFD)] whose junctions form no pair -> (input, (text, units, U+FFFD))"""
    data = b"".join(U.encode_units(p[0], order) if isinstance(p[0], list) else p[0][order] for p in pieces)
    text = b"".join(p[1] for p in pieces)
    n_units = sum(len(p[0]) if isinstance(p[0], list) else len(p[0][order]) // 2 for p in pieces)
    rep = sum(p[2] for p in pieces)
    if odd is not None:
        data, text, rep = data + bytes([odd]), text + U.FFFD, rep + 1
    return data, (text, n_units, rep)


def fill(ch, n):
    """n units of the BMP character ch as a piece, encoded once per byte order"""
    return ({U.LE: (ch * n).encode("utf-16-le"), U.BE: (ch * n).encode("utf-16-be")}, (ch * n).encode("utf-8"), 0)


PAIR = ([0xD83D, 0xDE00], "\U0001F600".encode("utf-8"), 0)
LONE_HIGH = ([0xDBFF], U.FFFD, 1)
LONE_LOW = ([0xDC00], U.FFFD, 1)


def straddling(n_units, boundaries, special, ch):
    """n_units units of ch with `special` placed at every boundary (a unit index) so that it straddles it: a pair has its high
    surrogate in front of the boundary and its low one behind it, a lone high is the last unit in front, a lone low the first behind"""
    pieces, at = [], 0
    for b in sorted(boundaries):
        start = b if special is LONE_LOW else b - 1
        if start < at or start + len(special[0]) > n_units:
            continue
        pieces += [fill(ch, start - at), special]
        at = start + len(special[0])
    pieces.append(fill(ch, n_units - at))
    return pieces


@pytest.mark.parametrize("kind", ["pair", "lone high", "lone low"])
def test_boundaries(env, kind):
    """(b): inputs of T - 2, T, T + 2 and 2 T C + T + 3 bytes with a surrogate pair, a lone high and a lone low surrogate across lane
    boundaries, tile boundaries and the boundaries between the workgroups of the prefix step, among ASCII (the neighbouring tiles take
    the fast path) and among three-byte units"""
    T, Cn = env.T, env.C
    special = {"pair": PAIR, "lone high": LONE_HIGH, "lone low": LONE_LOW}[kind]
    lane, tile, group = 8, T // 2, T * Cn // 2
    for n_bytes in (T - 2, T, T + 2, 2 * T * Cn + T + 3):
        n_units = n_bytes // 2
        marks = [lane, 5 * lane, 63 * lane, tile, tile + lane, n_units - 1, n_units] + [k * tile for k in (2, 3, 7, Cn - 1, Cn + 1)] + [group, 2 * group, group + tile, group - lane]
        marks = sorted({m for m in marks if 0 < m <= n_units})
        # every other mark only: two specials never touch, and tiles without one stay in between
        for ch in ("a", A3):
            for order in (U.LE, U.BE):
                for phase in (0, 1):
                    data, want = build(straddling(n_units, marks[phase::2], special, ch), order, odd=0xDC if n_bytes % 2 else None)
                    assert len(data) == n_bytes
                    if n_bytes <= T + 2:
                        assert want == U.reference(data, order)   # the construction against the oracle, where that is quick
                    check(env, data, order, want, f"{kind} in {n_bytes} bytes of {ch!r}, {U.CODEC[order]}, phase {phase}")


def test_construction_against_the_oracle(env):
    """the pieces of test_boundaries put together as the reference would, on a size the pure-Python reference walks quickly"""
    T = env.T
    for special in (PAIR, LONE_HIGH, LONE_LOW):
        for order in (U.LE, U.BE):
            data, want = build(straddling(3 * T // 2 + 1, [8, T // 2, T, 3 * T // 2 + 1], special, A3), order, odd=0x00)
            assert want == U.reference(data, order)
            check(env, data, order, want, "construction")


def test_every_output_residue(env):
    """(c): for each residue of a tile's output offset modulo 16: a general tile that shifts the output by the residue, an all-ASCII
    tile (fast path), a tile of three-byte units and another all-ASCII tile, then a ragged end: edge byte stores against interior wide
    stores, and the fast path next to the general path"""
    half = env.T // 2
    for r in range(16):
        for order in (U.LE, U.BE):
            pieces = [fill("é", r), fill("b", half - r), fill("a", half), fill(A3, half), fill("c", half), fill("d", 5 + r)]
            data, want = build(pieces, order)
            assert len(build(pieces[:2], order)[1][0]) % 16 == r   # the output offset of the first all-ASCII tile
            assert want == U.reference(data, order)
            check(env, data, order, want, f"residue {r} {U.CODEC[order]}")


def test_maximum_expansion(env):
    """(d): len / 2 units of U+FFFF, and of pairs; (e): the same with an odd last byte"""
    n = 3 * env.T // 2 + 10

    def run(pieces, order, odd, what):
        data, want = build(pieces, order, odd)
        check(env, data, order, want, f"{what} {U.CODEC[order]} odd byte {odd}")

    for order in (U.LE, U.BE):
        for odd in (None, 0xFF):
            run([fill("\uffff", n)], order, odd, "ffff")
            pairs = ([0xDBFF, 0xDFFF] * (n // 2), "\U0010FFFF".encode("utf-8") * (n // 2), 0)
            run([pairs], order, odd, "pairs")
            run([fill("a", 1), pairs], order, odd, "pairs shifted by a unit")
            run([([0xDC00] * n, U.FFFD * n, n)], order, odd, "lone lows")
            # the most one tile can give: three-byte units and a pair across its end
            run([fill(A3, env.T // 2 - 1), PAIR, fill(A3, env.T // 2 - 1), PAIR, fill(A3, 40)], order, odd, "full tiles with a pair across")


def test_device_input(env):
    """the input may lie in device memory: aligned it is read in place, unaligned it is copied first"""
    text = U.log_text(300, seed=3)
    data = text.encode("utf-16-le")
    dptr = on_device(np.frombuffer(b"\0" * 2 + data, dtype=np.uint8))
    try:
        for shift in (0, 2):
            raw = b"\0" * 2 + data
            r = env.sc.scan_utf16(dptr.value + shift, U.LE, want_text=True, nbytes=len(raw) - shift)
            assert r.utf16()["text"] == raw[shift:].decode("utf-16-le").encode("utf-8")
            r.close()
    finally:
        hip().hipFree(dptr)


# ---------------------------------------------------------------------------------------------------------------- records
INDICATORS = ["10.1.2.5", "10.1.2.77", "192.0.2.7", "198.51.100.9", "evil.example.com", "cdn3.bad.example.org", G.MD5, "203.0.113.4", "www.example.net"]


def snapshot(res, text, mode):
    """everything a host-resident result says, in an order that does not depend on the order of an unsorted fetch"""
    s = dict(n_hits=res.n_hits, lines=res.lines, candidates=res.candidates, bytes=res.bytes, lines_with_matches=res.lines_with_matches)
    hl = res.hit_lines()
    s["hl_n_lines"] = hl["n_lines"]
    if mode == COUNTS:
        return s
    s["block"] = (hl["text"], hl["line_off"].tolist(), hl["line_no"].tolist())
    hits = res.hits()
    lines = res.ip4_lines + res.line_records
    of = ([] if hl["line_of_ip4_hit"] is None else hl["line_of_ip4_hit"].tolist()) + hl["line_of_hit"].tolist()
    assert len(hits) == len(lines) == len(of) == res.n_hits
    s["records"] = sorted((h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"]), tuple(h["offs"]), l,
                           hl["text"][hl["line_off"][k]:hl["line_off"][k + 1]]) for h, l, k in zip(hits, lines, of))
    s["rendered"] = sorted(res.rendered_ndjson().split(b"\n"))
    s["host_lines"] = sorted(res.ndjson_lines_text(text, source=SOURCE, line_base=LINE_BASE, with_input_line=True).split(b"\n"))
    s["host_from_block"] = sorted(res.ndjson_lines_text(None, source=SOURCE, line_base=LINE_BASE, with_input_line=True).split(b"\n"))
    s["host_plain"] = sorted(res.ndjson_text(text, source=SOURCE).split(b"\n"))
    s["single"] = sorted(res.ndjson(text, source=SOURCE))
    return s


@pytest.fixture(scope="module")
def reference_run(env):
    """the UTF-8 text through matchy_scanner_scan with line context, hit lines, rendered records and the tally: once, shared"""
    text = U.log_text(3000, seed=11, indicators=INDICATORS)
    utf8 = text.encode("utf-8")
    M, sc = env.M, env.ref
    sc.set_line_context(True); sc.set_hit_lines(True); sc.set_tally(True); sc.reset_tally()
    sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
    r = sc.scan(utf8)
    snap = snapshot(r, utf8, SORTED)
    r.close()
    tally = list(sc.tally())
    sc.set_tally(False); sc.set_line_context(False); sc.set_hit_lines(False)
    assert snap["n_hits"] > 1000 and {x[3] for x in snap["records"]} == {"ip", "pattern"} and any("€".encode() in x[-1] or b"\xf0" in x[-1] for x in snap["records"])
    return dict(text=text, utf8=utf8, snap=snap, tally=tally)


@pytest.mark.parametrize("order", [U.LE, U.BE], ids=["le", "be"])
@pytest.mark.parametrize("mode", [COUNTS, HITS, SORTED, COMPACT, DEVICE], ids=["counts", "hits", "sorted", "compact", "device"])
def test_records_equal_the_utf8_scan(env, reference_run, mode, order):
    """(f): hits, pattern ids, data offsets, lines, candidates, line records, the tally, the block of hit lines, the rendered NDJSON block
    and the NDJSON of the host calls equal those of matchy_scanner_scan over the UTF-8 text"""
    M, sc, want, utf8 = env.M, env.sc, reference_run["snap"], reference_run["utf8"]
    data = reference_run["text"].encode(U.CODEC[order])
    sc.set_line_context(True); sc.set_hit_lines(True); sc.set_tally(True); sc.reset_tally()
    sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
    try:
        r = sc.scan_utf16(data, order, want_text=mode != DEVICE, fetch_mode=mode)
        u = r.utf16()
        assert (u["text_len"], u["code_units"], u["replaced"]) == (len(utf8), len(data) // 2, 0)
        assert (r.n_hits, r.lines, r.candidates, r.bytes, r.lines_with_matches) == (want["n_hits"], want["lines"], want["candidates"], len(utf8), want["lines_with_matches"])
        assert list(sc.tally()) == reference_run["tally"]
        if mode == DEVICE:
            assert r.on_device and u["text"] is None
            starts, lines, recs, _ = read(r)
            assert sorted(zip(starts.tolist(), (recs["len_type"] & 0xFFFFFF).tolist(), map(tuple, lines[:, :3].tolist()))) == \
                sorted((x[0], x[1] - x[0], x[8]) for x in want["records"])
            assert r.hit_lines()["n_lines"] == want["hl_n_lines"] and r.rendered_ndjson()[1] == sum(len(x) + 1 for x in want["rendered"] if x)
        else:
            assert u["text"] == utf8
            got = snapshot(r, u["text"], mode)
            assert (r.n_ip4_hits > 0) == (mode == COMPACT)
            for k in got:
                assert got[k] == want[k], k
            if mode == SORTED:
                starts = [h["start"] for h in r.hits()]
                assert starts == sorted(starts)
        r.close()
    finally:
        sc.set_tally(False); sc.set_line_context(False); sc.set_hit_lines(False)


def test_multi_scanner(env, reference_run):
    """(f) through matchy_multi_scanner_submit_utf16: two batches, one per byte order, with and without the text"""
    M, want, utf8 = env.M, reference_run["snap"], reference_run["utf8"]
    le, be = reference_run["text"].encode("utf-16-le"), reference_run["text"].encode("utf-16-be")
    keep = [C.create_string_buffer(le, len(le)), C.create_string_buffer(be, len(be))]
    ms = M.MultiScanner(env.db, devices=(0,))
    try:
        ms.set_line_context(True); ms.set_hit_lines(True); ms.set_tally(True)
        for k, order in enumerate((U.LE, U.BE)):
            ms.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
            ms.submit_utf16_ptr(C.addressof(keep[k]), len(le), order, want_text=k == 0, tag=k)
        for k in range(2):
            b = ms.next(want_hits=True)
            assert (b["tag"], b["n_hits"], b["lines"], b["candidates"], b["nbytes"]) == (k, want["n_hits"], want["lines"], want["candidates"], len(utf8))
            assert b["text"] == (utf8 if k == 0 else None)
            assert b["utf16"] == dict(text_len=len(utf8), code_units=len(le) // 2, replaced=0)
            assert b["lines_with_matches"] == want["lines_with_matches"]
            assert sorted((h["start"], h["end"], h["type"], tuple(h["ids"]), tuple(h["offs"]), l) for h, l in zip(b["hits"], b["line_records"])) == \
                sorted((x[0], x[1], x[2], x[6], x[7], x[8]) for x in want["records"])
            assert (b["hit_lines"]["text"], b["hit_lines"]["line_off"].tolist(), b["hit_lines"]["line_no"].tolist()) == want["block"]
            assert sorted(b["rendered"].split(b"\n")) == want["rendered"]
        assert ms.next() is None
        assert [(t, ty, 2 * c) for t, ty, c in reference_run["tally"]] == list(ms.tally())
        # the parameter errors of the submit call
        L = M.lib()
        assert L.matchy_multi_scanner_submit_utf16(ms._h, C.addressof(keep[0]), len(le), 2, False, None, None) == INVALID and "byte_order" in M.last_error()
        assert L.matchy_multi_scanner_submit_utf16(None, C.addressof(keep[0]), len(le), 0, False, None, None) == INVALID
        assert L.matchy_multi_scanner_submit_utf16(ms._h, C.addressof(keep[0]), (1 << 31) // 3 * 2 + 2, 0, False, None, None) == INVALID and "2^31" in M.last_error()
        assert ms.pending() == 0
    finally:
        ms.close()


def test_parameter_errors_leave_the_scanner_usable(env):
    """(h): NULL handles, a byte order above 1, the 2^31 bound, a pending segment table and whole-line mode: MATCHY_ERROR_INVALID_PARAM
    with a message, nothing launched, and the next scan succeeds"""
    M, sc = env.M, env.sc
    L = M.lib()
    data = "src=10.1.2.5 € evil.example.com\n".encode("utf-16-le")
    want = (data.decode("utf-16-le").encode("utf-8"), len(data) // 2, 0)

    def works():
        r = sc.scan_utf16(data, U.LE, want_text=True, fetch_mode=HITS)
        assert (r.utf16()["text"], r.utf16()["code_units"], r.utf16()["replaced"]) == want and r.n_hits == 2
        r.close()

    works()
    raw = M._ScanResult()
    assert L.matchy_scanner_scan_utf16(None, data, len(data), 0, HITS, False, C.byref(raw)) == INVALID
    assert L.matchy_scanner_scan_utf16(sc._h, data, len(data), 0, HITS, False, None) == INVALID
    assert L.matchy_scanner_scan_utf16(sc._h, None, 4, 0, HITS, False, C.byref(raw)) == INVALID
    works()
    with pytest.raises(RuntimeError, match="byte_order"):
        sc.scan_utf16(data, 2)
    works()
    # the bound 3 * (len / 2) + 3 * (len & 1) reaches 2^31: refused by the length alone, nothing is read
    first_refused = next(n for n in range((1 << 31) // 3 * 2 - 4, (1 << 31) // 3 * 2 + 8) if 3 * (n // 2) + 3 * (n & 1) >= 1 << 31)
    assert 3 * ((first_refused - 1) // 2) + 3 * ((first_refused - 1) & 1) < 1 << 31
    assert L.matchy_scanner_scan_utf16(sc._h, data, first_refused, 0, HITS, False, C.byref(raw)) == INVALID and "2^31" in M.last_error()
    works()
    sc.set_segments([0, 4])
    with pytest.raises(RuntimeError, match="segments"):
        sc.scan_utf16(data, U.LE)
    works()   # the pending table was dropped
    sc.set_whole_lines(True)
    try:
        with pytest.raises(RuntimeError, match="whole-line"):
            sc.scan_utf16(data, U.LE)
    finally:
        sc.set_whole_lines(False)
    works()
    # a result of another kind of scan
    r = sc.scan(want[0])
    assert r.utf16() is None and L.matchy_scan_result_utf16(C.byref(r._raw), None, None, None, None) == INVALID and "UTF-16" in M.last_error()
    r.close()
    assert L.matchy_scan_result_utf16(None, None, None, None, None) == INVALID


def test_timing(env):
    """the three steps report times, and a scanner that never transcoded reports zeros"""
    M = env.M
    sc = M.Scanner(env.db)
    try:
        assert sc.utf16_timing_ms() == (0.0, 0.0, 0.0)
        data = U.log_text(2000, seed=5).encode("utf-16-le")
        r = sc.scan_utf16(data, U.LE)
        r.close()
        t = sc.utf16_timing_ms()
        print("utf16 count / prefix / write ms:", t)
        assert all(x > 0 for x in t)
    finally:
        sc.close()
