"""GPU: percent- and JSON-escaped inputs (matchy_scanner_scan_escaped, csrc/unescape.hip). Expected bytes come from the pure-Python
reference of tests/unescape_cases.py, which tests/test_unescape_host.py holds against urllib, json and the CPU driver of the same
rules; expected records come from the existing path: matchy_scanner_scan of the decoded text. Shapes follow
matchy_amd_unescape_geometry: T the tile bytes, C the tiles of a workgroup of the prefix step, S those of the state scan."""
import ctypes as C
import random

import numpy as np
import pytest

import gz_cases as G
import unescape_cases as U
from test_gpu_line_context import hip, on_device, read
from test_gpu_utf16 import INDICATORS, LINE_BASE, SOURCE, snapshot

pytestmark = pytest.mark.gpu

COUNTS, HITS, SORTED, COMPACT, DEVICE = 0, 1, 3, 1 | 8, 4
INVALID = -5
P, J, B = U.PERCENT, U.JSON, U.PERCENT | U.JSON
MODE_NAME = {P: "percent", J: "json", B: "json+percent"}


class Env:
    def __init__(self):
        import matchy_amd as M
        self.M = M
        self.db = M.Database(G.blob())
        self.sc = M.Scanner(self.db)      # escaped scans
        self.ref = M.Scanner(self.db)     # the reference: scans of the decoded text
        self.T, self.C, self.S = M.unescape_geometry()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.sc.close(); e.ref.close(); e.db.close()


def decode(env, data, modes, fetch_mode=COUNTS, nbytes=None):
    """(text, escapes, replaced, lf_escapes) of one call with want_text, the result's own figures checked against each other"""
    r = env.sc.scan_escaped(data, modes, want_text=True, fetch_mode=fetch_mode, nbytes=nbytes)
    u = r.unescaped()
    assert u is not None and u["text"] is not None and u["text_len"] == len(u["text"]) == r.bytes
    assert r.lines == u["text"].count(b"\n")
    r.close()
    return u["text"], u["escapes"], u["replaced"], u["lf_escapes"]


def check(env, data, modes, want, what):
    got = decode(env, data, modes)
    text = got[0]
    if text != want[0]:   # name the first difference instead of printing megabytes
        n = min(len(text), len(want[0]))
        at = next((i for i in range(n) if text[i] != want[0][i]), n)
        raise AssertionError(f"{what}: text differs at byte {at} (lengths {len(text)}, {len(want[0])}): {text[max(at - 8, 0):at + 8]!r} for {want[0][max(at - 8, 0):at + 8]!r}")
    assert got[1:] == tuple(want[1:]), what


def test_geometry(env):
    assert env.T == 1024 and env.C >= 2 and env.S >= 2 and env.T % 16 == 0
    assert (env.M.UNESCAPE_PERCENT, env.M.UNESCAPE_JSON) == (P, J)


@pytest.mark.parametrize("modes", [P, J, B], ids=lambda m: MODE_NAME[m])
def test_every_case_in_its_own_call(env, modes):
    """every named and generated case in its own call under each of the three modes; then all of them joined with LF as one input"""
    cases = [(name, data) for name, _, data, _ in U.named_cases()] + [(f"generated {k}", data) for k, (_, data) in enumerate(U.generated_cases())]
    assert len(cases) > 4000
    for name, data in cases:
        check(env, data, modes, U.reference(data, modes), f"{name} as {MODE_NAME[modes]}")
    joined = b"\n".join(data for _, data in cases)
    assert len(joined) > 8 * env.T
    check(env, joined, modes, U.reference(joined, modes), f"all cases joined, {MODE_NAME[modes]}")


def test_named_cases_give_the_bytes_written_by_hand(env):
    for name, modes, data, text in U.named_cases():
        assert decode(env, data, modes)[0] == text, name


# ------------------------------------------------------------------------------------------------ constructed inputs
# a piece: (input, text, escapes, U+FFFD, LF escapes); the junctions of the pieces of an input form no escape
def build(pieces):
    data = b"".join(p[0] for p in pieces)
    return data, (b"".join(p[1] for p in pieces), sum(p[2] for p in pieces), sum(p[3] for p in pieces), sum(p[4] for p in pieces))


def plain(n, ch=b"a"):
    return (ch * n, ch * n, 0, 0, 0)


def dense_json(n):
    """n bytes of \\u00e9 escapes, padded with x to the length"""
    k, pad = divmod(n, 6)
    return (b"\\u00e9" * k + b"x" * pad, "é".encode() * k + b"x" * pad, k, 0, 0)


def dense_percent(n):
    k, pad = divmod(n, 6)
    return (b"%c3%a9" * k + b"x" * pad, "é".encode() * k + b"x" * pad, 2 * k, 0, 0)


KINDS = {
    "%41": (P, (b"%41", b"A", 1, 0, 0)),
    "\\/": (J, (b"\\/", b"/", 1, 0, 0)),
    "\\u20ac": (J, (b"\\u20ac", "€".encode(), 1, 0, 0)),
    "pair": (J, (b"\\ud83d\\ude00", "\U0001F600".encode(), 2, 0, 0)),
    "lone high": (J, (b"\\udbff", U.FFFD, 1, 1, 0)),
    "lone low": (J, (b"\\udc00", U.FFFD, 1, 1, 0)),
}


def straddling(n, marks, special, split_of, fill):
    """n bytes of filler with `special` placed at every mark so that split_of(i) of its bytes lie in front of mark i"""
    pieces, at = [], 0
    for i, m in enumerate(sorted(marks)):
        start = m - split_of(i)
        if start < at + 1 or start + len(special[0]) > n:   # one byte of filler at least between two specials
            continue
        pieces += [fill(start - at), special]
        at = start + len(special[0])
    pieces.append(fill(n - at))
    return pieces


@pytest.mark.parametrize("kind", list(KINDS))
def test_boundaries(env, kind):
    """inputs of T - 1, T, T + 1 and 2 T C + T + 3 bytes with one kind of escape across lane boundaries, tile boundaries and the
    boundaries between the workgroups of the prefix step, with every split point of the escape at every boundary, among escape-free
    filler (the neighbouring tiles take the fast path) and among dense filler (they do not)"""
    T, Cn = env.T, env.C
    modes, special = KINDS[kind]
    n_split = len(special[0]) - 1
    tile, group = T, T * Cn
    for n in (T - 1, T, T + 1, 2 * T * Cn + T + 3):
        marks = [16, 32, 5 * 16, 62 * 16, 63 * 16, tile, tile + 16, n] + [k * tile for k in (2, 3, 7, Cn - 1, Cn + 1)] + [group, 2 * group, group + tile, group - 16]
        marks = sorted({m for m in marks if 0 < m <= n})
        for fill in (plain, dense_percent if modes == P else dense_json):
            for phase in range(n_split):
                data, want = build(straddling(n, marks, special, lambda i: 1 + (i + phase) % n_split, fill))
                assert len(data) == n
                if n <= T + 1:
                    assert want == U.reference(data, modes)   # the construction against the oracle, where that is quick
                check(env, data, modes, want, f"{kind} in {n} bytes of {fill.__name__}, phase {phase}")


def test_construction_against_the_oracle(env):
    """the pieces of test_boundaries put together as the reference would, on a size the pure-Python reference walks quickly"""
    T = env.T
    for kind, (modes, special) in KINDS.items():
        for fill in (plain, dense_percent if modes == P else dense_json):
            for phase in range(len(special[0]) - 1):
                data, want = build(straddling(3 * T + 5, [16, T, 2 * T, 3 * T, 3 * T + 5], special, lambda i: 1 + (i + phase) % (len(special[0]) - 1), fill))
                assert want == U.reference(data, modes)
                check(env, data, modes, want, f"construction {kind}")


def test_backslash_runs_at_a_tile_boundary(env):
    """runs of 1 to 40 backslashes followed by n, ending at every offset from T - 42 to T + 2: an even run is backslashes and an n, an
    odd one ends in an escape for LF"""
    T = env.T
    for run in range(1, 41):
        for end in range(T - 42, T + 3):
            data = b"a" * (end - run) + b"\\" * run + b"n" + b"b" * 20
            want = (b"a" * (end - run) + b"\\" * (run // 2) + (b" " if run & 1 else b"n") + b"b" * 20, (run + 1) // 2, 0, run & 1)
            check(env, data, J, want, f"run of {run} ending at {end}")


def run_piece(run, tail):
    """`run` backslashes and `tail` (b"n" or b"")"""
    if tail and run & 1:
        return (b"\\" * run + tail, b"\\" * (run // 2) + b" ", run // 2 + 1, 0, 1)
    return (b"\\" * run + tail, b"\\" * ((run + 1) // 2) + tail, run // 2, 0, 0)   # an odd run without n: its last backslash is the input's last byte


def test_long_backslash_runs(env):
    """runs of exactly T, 2 T + 1 and 3 T backslashes that start at offsets 0, 1 and T - 1, with and without an n behind them"""
    T = env.T
    for run in (T, 2 * T + 1, 3 * T):
        for start in (0, 1, T - 1):
            for tail in (b"n", b""):
                data, want = build([plain(start), run_piece(run, tail)])
                assert want == U.reference(data, J)
                check(env, data, J, want, f"run of {run} at {start} + {tail!r}")
                if tail:   # something behind the run, so that the tiles behind it depend on its parity too
                    data, want = build([plain(start), run_piece(run, tail), plain(T + 7), KINDS["pair"][1], plain(3)])
                    check(env, data, J, want, f"run of {run} at {start} + n + a tile")


def test_backslashes_only_and_linear_time(env):
    """one input of backslashes only of 2 T S + T + 1 bytes, and the same plus n. The O(n) check: the three step times stay within 10x
    those of an escape-free input of the same length — the dense path is dearer than the copy path; a walk back from every tile to the
    start of the run would be thousands of times slower"""
    n = 2 * env.T * env.S + env.T + 1
    M = env.M
    sc = M.Scanner(env.db)
    try:
        def timed(data, want):
            best = None
            for _ in range(3):
                r = sc.scan_escaped(data, J, want_text=True, fetch_mode=COUNTS)
                u = r.unescaped()
                assert (u["text"], u["escapes"], u["replaced"], u["lf_escapes"]) == want
                r.close()
                t = sc.unescape_timing_ms()
                best = t if best is None else tuple(min(a, b) for a, b in zip(best, t))
            return best
        free = timed(b"a" * n, (b"a" * n, 0, 0, 0))
        runs = timed(*build([run_piece(n, b"")]))
        runs_n = timed(*build([run_piece(n, b"n")]))
        print(f"count / prefix / write ms for {n} bytes: escape-free {free}, backslashes only {runs}, backslashes and n {runs_n}")
        for k in range(3):
            assert runs[k] <= 10 * free[k] and runs_n[k] <= 10 * free[k], (k, free, runs, runs_n)
    finally:
        sc.close()


@pytest.mark.parametrize("modes", [P, J], ids=lambda m: MODE_NAME[m])
def test_every_output_residue(env, modes):
    """for each residue of a tile's output offset modulo 16: a general tile that shortens the output by the residue, an escape-free tile
    (fast path), a dense tile and another escape-free tile, then a ragged end: edge byte stores against interior wide stores, and the
    fast path next to the general path"""
    T = env.T
    esc = KINDS["%41"][1] if modes == P else KINDS["\\/"][1]
    dense = dense_percent if modes == P else dense_json
    seen = set()
    for r in range(16):
        first = [esc] * r + [plain(T - r * len(esc[0]), b"b")]
        pieces = first + [plain(T), dense(T), plain(T, b"c"), plain(5 + r, b"d")]
        data, want = build(pieces)
        assert len(build(first)[0]) == T
        seen.add(len(build(first)[1][0]) % 16)   # the output offset of the first escape-free tile
        assert want == U.reference(data, modes)
        check(env, data, modes, want, f"residue {r} {MODE_NAME[modes]}")
    if modes == J:
        assert len(seen) == 16
        return
    # %41 shortens by 2, and an escape-free tile has no escape across its first byte, so its offset is even. The odd residues belong to
    # general tiles: an escape with one byte behind the tile's first boundary
    assert seen == set(range(0, 16, 2))
    for r in range(8):
        first = [esc] * r + [plain(T - 2 - r * len(esc[0]), b"b")]
        data, want = build(first + [esc, plain(T - 1), dense(T), plain(T, b"c"), plain(5 + r, b"d")])
        assert len(build(first)[0]) == T - 2 and (len(build(first)[1][0]) + 1) % 16 == 15 - 2 * r
        assert want == U.reference(data, modes)
        check(env, data, modes, want, f"odd residue {15 - 2 * r}")


def test_device_input(env):
    """the input may lie in device memory: aligned it is read in place, unaligned it is copied first"""
    data = b"".join(rng_line for rng_line in mixed_log(400, seed=3))
    raw = b"\n\n" + data
    dptr = on_device(np.frombuffer(raw, dtype=np.uint8))
    try:
        for shift in (0, 1, 2):
            got = decode(env, dptr.value + shift, B, nbytes=len(raw) - shift)
            assert got == U.reference(raw[shift:], B), shift
    finally:
        hip().hipFree(dptr)


# ---------------------------------------------------------------------------------------------------------------- records
def pct(s):
    return "".join(f"%{ord(ch):02X}" if ch in ":/.?=&" and k % 3 else ch for k, ch in enumerate(s))


def mixed_log(n_lines, seed):
    """the lines (bytes, each with its LF) of a log whose indicators come raw, percent-encoded, inside nested JSON and with \\/ and \\u002e"""
    rng = random.Random(seed)
    lines = []
    for i in range(n_lines):
        ind, ind2 = rng.choice(INDICATORS), rng.choice(INDICATORS)
        shape = rng.randrange(40)
        if shape == 0:
            line = f"10.9.8.7 - - \"GET /r?url=https%3A%2F%2F{ind}%2Fpath&a={pct(ind2)}%0Anext HTTP/1.1\" 302 {i}"
        elif shape == 1:
            line = '{"ts":%d,"msg":"{\\"host\\":\\"%s\\",\\"peer\\":\\"%s\\"}"}' % (i, ind, ind2)
        elif shape == 2:
            line = '{"msg":"line1\\n%s\\tnext","u":"https:\\/\\/%s\\/x","e":"%s","smile":"\\ud83d\\ude00 caf\\u00e9"}' % (ind, ind2, ind.replace(".", "\\u002e"))
        elif shape == 3:
            line = f"raw src={ind} dst={ind2} café"
        else:
            line = f"2026-01-{1 + i % 28:02d}T10:{i % 60:02d}:00Z host{i % 13} req={rng.randrange(1 << 30):08x} " + "nothing to see here, " * rng.randint(2, 9) + "done"
        lines.append(line.encode("utf-8") + b"\n")
    return lines


@pytest.fixture(scope="module")
def reference_run(env):
    """a mixed log of about 3 T C bytes, its decoded text from the reference, and that text through matchy_scanner_scan with line
    context, hit lines, rendered records and the tally: once, shared"""
    lines, size = [], 0
    for line in mixed_log(200000, seed=11):
        lines.append(line)
        size += len(line)
        if size >= 3 * env.T * env.C:
            break
    raw = b"".join(lines)
    text, escapes, replaced, lf = U.reference(raw, B)
    assert escapes > 1000 and lf > 10 and text.count(b"\n") == raw.count(b"\n")
    M, sc = env.M, env.ref
    r = sc.scan(raw)
    raw_hits = r.n_hits
    r.close()
    sc.set_line_context(True); sc.set_hit_lines(True); sc.set_tally(True); sc.reset_tally()
    sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
    r = sc.scan(text)
    snap = snapshot(r, text, SORTED)
    r.close()
    tally = list(sc.tally())
    sc.set_tally(False); sc.set_line_context(False); sc.set_hit_lines(False)
    assert snap["n_hits"] > 1000 and {x[3] for x in snap["records"]} == {"ip", "pattern"}
    return dict(raw=raw, text=text, counters=(escapes, replaced, lf), snap=snap, tally=tally, raw_hits=raw_hits)


@pytest.mark.parametrize("mode", [COUNTS, HITS, SORTED, COMPACT, DEVICE], ids=["counts", "hits", "sorted", "compact", "device"])
def test_records_equal_the_scan_of_the_decoded_text(env, reference_run, mode):
    """hits, pattern ids, data offsets, lines, candidates, line records, the tally, the block of hit lines, the rendered NDJSON block
    and the NDJSON of the host calls equal those of matchy_scanner_scan over the reference's decoded text; the raw bytes give fewer hits"""
    M, sc, want, text = env.M, env.sc, reference_run["snap"], reference_run["text"]
    assert reference_run["raw_hits"] < want["n_hits"]
    sc.set_line_context(True); sc.set_hit_lines(True); sc.set_tally(True); sc.reset_tally()
    sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
    try:
        r = sc.scan_escaped(reference_run["raw"], B, want_text=mode != DEVICE, fetch_mode=mode)
        u = r.unescaped()
        assert (u["text_len"], u["escapes"], u["replaced"], u["lf_escapes"]) == (len(text),) + reference_run["counters"]
        assert (r.n_hits, r.lines, r.candidates, r.bytes, r.lines_with_matches) == (want["n_hits"], want["lines"], want["candidates"], len(text), want["lines_with_matches"])
        assert list(sc.tally()) == reference_run["tally"]
        if mode == DEVICE:
            assert r.on_device and u["text"] is None
            starts, lines, recs, _ = read(r)
            assert sorted(zip(starts.tolist(), (recs["len_type"] & 0xFFFFFF).tolist(), map(tuple, lines[:, :3].tolist()))) == \
                sorted((x[0], x[1] - x[0], x[8]) for x in want["records"])
            assert r.hit_lines()["n_lines"] == want["hl_n_lines"] and r.rendered_ndjson()[1] == sum(len(x) + 1 for x in want["rendered"] if x)
        else:
            assert u["text"] == text
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
    """through matchy_multi_scanner_submit_escaped: two batches, with and without the text"""
    M, want, text, raw = env.M, reference_run["snap"], reference_run["text"], reference_run["raw"]
    keep = C.create_string_buffer(raw, len(raw))
    ms = M.MultiScanner(env.db, devices=(0,))
    try:
        ms.set_line_context(True); ms.set_hit_lines(True); ms.set_tally(True)
        for k in range(2):
            ms.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source=SOURCE, line_base=LINE_BASE)
            ms.submit_escaped(C.addressof(keep), len(raw), B, want_text=k == 0, tag=k)
        for k in range(2):
            b = ms.next(want_hits=True)
            assert (b["tag"], b["n_hits"], b["lines"], b["candidates"], b["nbytes"]) == (k, want["n_hits"], want["lines"], want["candidates"], len(text))
            assert b["text"] == (text if k == 0 else None)
            assert b["unescaped"] == dict(zip(("text_len", "escapes", "replaced", "lf_escapes"), (len(text),) + reference_run["counters"]))
            assert b["lines_with_matches"] == want["lines_with_matches"]
            assert sorted((h["start"], h["end"], h["type"], tuple(h["ids"]), tuple(h["offs"]), l) for h, l in zip(b["hits"], b["line_records"])) == \
                sorted((x[0], x[1], x[2], x[6], x[7], x[8]) for x in want["records"])
            assert (b["hit_lines"]["text"], b["hit_lines"]["line_off"].tolist(), b["hit_lines"]["line_no"].tolist()) == want["block"]
            assert sorted(b["rendered"].split(b"\n")) == want["rendered"]
        assert ms.next() is None
        assert [(t, ty, 2 * c) for t, ty, c in reference_run["tally"]] == list(ms.tally())
        # the parameter errors of the submit call
        L = M.lib()
        assert L.matchy_multi_scanner_submit_escaped(ms._h, C.addressof(keep), len(raw), 0, False, None, None) == INVALID and "modes" in M.last_error()
        assert L.matchy_multi_scanner_submit_escaped(ms._h, C.addressof(keep), len(raw), 4, False, None, None) == INVALID and "modes" in M.last_error()
        assert L.matchy_multi_scanner_submit_escaped(None, C.addressof(keep), len(raw), 1, False, None, None) == INVALID
        assert L.matchy_multi_scanner_submit_escaped(ms._h, C.addressof(keep), 0x7FFF0000, 1, False, None, None) == INVALID and "2^31" in M.last_error()
        assert ms.pending() == 0
    finally:
        ms.close()


def test_parameter_errors_leave_the_scanner_usable(env):
    """NULL handles, modes 0 and above 3, no input, the length bound, a pending segment table and whole-line mode:
    MATCHY_ERROR_INVALID_PARAM with a message, nothing launched, and the next scan succeeds"""
    M, sc = env.M, env.sc
    L = M.lib()
    data = b'{"m":"src=10.1.2.5 \\u20ac evil%2Eexample%2Ecom\\n"}\n'
    want = U.reference(data, B)
    assert b"evil.example.com " in want[0]

    def works():
        r = sc.scan_escaped(data, B, want_text=True, fetch_mode=HITS)
        u = r.unescaped()
        assert (u["text"], u["escapes"], u["replaced"], u["lf_escapes"]) == want and r.n_hits == 2
        r.close()

    works()
    raw = M._ScanResult()
    assert L.matchy_scanner_scan_escaped(None, data, len(data), 1, HITS, False, C.byref(raw)) == INVALID
    assert L.matchy_scanner_scan_escaped(sc._h, data, len(data), 1, HITS, False, None) == INVALID
    assert L.matchy_scanner_scan_escaped(sc._h, None, 4, 1, HITS, False, C.byref(raw)) == INVALID and "no input" in M.last_error()
    works()
    for modes in (0, 4, 7):
        with pytest.raises(RuntimeError, match="modes"):
            sc.scan_escaped(data, modes)
        works()
    # refused by the length alone, nothing is read
    assert L.matchy_scanner_scan_escaped(sc._h, data, 0x7FFF0000, 1, HITS, False, C.byref(raw)) == INVALID and "2^31" in M.last_error()
    works()
    sc.set_segments([0, 4])
    with pytest.raises(RuntimeError, match="segments"):
        sc.scan_escaped(data, J)
    works()   # the pending table was dropped
    sc.set_whole_lines(True)
    try:
        with pytest.raises(RuntimeError, match="whole-line"):
            sc.scan_escaped(data, J)
    finally:
        sc.set_whole_lines(False)
    works()
    # a result of another kind of scan
    r = sc.scan(want[0])
    assert r.unescaped() is None and L.matchy_scan_result_unescaped(C.byref(r._raw), None, None, None) == INVALID and "escaped scan" in M.last_error()
    r.close()
    assert L.matchy_scan_result_unescaped(None, None, None, None) == INVALID
    # an empty input is a scan of nothing
    r = sc.scan_escaped(b"", B, want_text=True)
    assert r.unescaped()["text_len"] == 0 and r.n_hits == 0
    r.close()
    works()


def test_timing(env):
    """the three steps report times, and a scanner that never decoded reports zeros"""
    M = env.M
    sc = M.Scanner(env.db)
    try:
        assert sc.unescape_timing_ms() == (0.0, 0.0, 0.0)
        data = b"".join(mixed_log(3000, seed=5))
        for modes in (P, J, B):
            r = sc.scan_escaped(data, modes)
            r.close()
            t = sc.unescape_timing_ms()
            print(f"unescape {MODE_NAME[modes]} count / prefix / write ms:", t)
            assert all(x > 0 for x in t)
    finally:
        sc.close()
