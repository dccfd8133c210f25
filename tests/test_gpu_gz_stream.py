"""GPU: stream windows (matchy_scanner_scan_gz_stream; csrc/inflate_pieces.hip "stream windows"). One DEFLATE stream is scanned as a
chain of windows: every window hands the bit where it stopped, the state (length, CRC-32 and last 32 KiB of the text so far) and the
partial line behind its last newline to the next. The vectors and window sizes are those of tests/test_gz_stream_host.py, which runs
them through the same rules under a sanitizer first; here the CPU driver (tests/cpp/test_gz_stream.cpp, built as a plain program) gives
the expected consumed bits, text lengths, states and piece tables field for field, zlib the text, and the plain scan of the whole text
on a second scanner the records. A window's batch starts at the file offset of the bytes reported so far (its carry is the file's bytes
in front of its text), so batch offsets map to file offsets by adding that count."""
import ctypes as C

import pytest

import gz_cases as G
import gz_files_cases as F
import gz_pieces_cases as P
import gz_stream_cases as S
import test_gpu_gz as T
from test_gpu_gz_window import FETCH_COMPACT, FETCH_COUNTS, FETCH_DEVICE, FETCH_HITS, FETCH_SORTED, keyed, numbered, plain

pytestmark = pytest.mark.gpu

CARRY_CAP = 4096


@pytest.fixture(scope="module")
def env():
    e = T.Env()
    yield e
    e.sc.set_gz_pieces(0)
    e.sc.close(); e.ref.close(); e.db.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S.build_driver(tmp_path_factory.mktemp("gz_stream_gpu"))


@pytest.fixture(scope="module")
def cpu(driver, tmp_path_factory):
    """the CPU driver's chains, computed once per (file, chain): a function with a cache"""
    tmp, cache = tmp_path_factory.mktemp("gz_stream_cpu"), {}

    def get(gz, chain):
        key = (gz, chain)
        if key not in cache:
            cache[key] = S.run_chains(driver, tmp, [gz], chain, tag=str(len(cache)))[0]
        return cache[key]
    return get


def model_tail(full, ended, carry_cap):
    """(bytes reported, carry) of a batch whose carry and text are `full`: k_gz_window_tail's rule"""
    if ended:
        return len(full), b""
    cut = full.rfind(b"\n") + 1
    if cut == 0 and len(full) > carry_cap or len(full) - cut > carry_cap:
        return None
    return cut, full[cut:]


def run_chain(env, gz, chain, lines=False, fetch_mode=FETCH_HITS, sc=None, want_text=True, scan=None):
    """the windows of one file in order, as csrc/gz_stream.h walks them: [dict per window], records in file coordinates"""
    M, sc = env.M, sc or env.sc
    window_bytes, piece_bytes, text_cap = chain
    sc.set_gz_pieces(piece_bytes)
    sc.set_line_context(lines)
    walk = M.GzStreamWalker(len(gz), window_bytes, piece_bytes, text_cap)
    state, carry, shift, line_base, out = None, b"", 0, 0, []
    while not walk.over:
        w = walk.next()
        offset, length, bit, flags = w
        assert state is None or state.bit == bit
        if scan:
            r = scan(gz[offset:offset + length], state, carry, text_cap, flags)
        else:
            r = sc.scan_gz_stream(gz[offset:offset + length], state=state, carry=carry, carry_cap=CARRY_CAP, text_cap=text_cap, first=bool(flags & M.STREAM_FIRST),
                                  file_end=bool(flags & M.STREAM_FILE_END), want_text=want_text, fetch_mode=fetch_mode)
        v = r.gz_stream()
        g = dict(v, window=w, carry_in=carry, batch=r.gz_text(), batch_len=r.gz_text_len(), bytes=r.bytes, lines=r.lines, n_hits=r.n_hits, segments=r.segments,
                 member_status=r.gz_status(), pieces=r.gz_pieces(), shift=shift,
                 hits=keyed(r.hits(), shift) if fetch_mode & 1 and fetch_mode != FETCH_DEVICE else None,
                 numbered=numbered(r, shift, line_base) if lines and fetch_mode & 1 and fetch_mode != FETCH_DEVICE else None)
        r.close()
        out.append(g)
        if v["status"] != M.STREAM_OK:
            walk.refuse()
            break
        assert walk.accept(w, v["consumed_bits"], v["text_len"], v["ended"])
        state, carry, shift, line_base = v["state"], v["carry"], shift + g["bytes"], line_base + g["lines"]
    return out


def check_against_cpu(env, got, want, text_cap, with_text=True):
    """every window of the GPU chain against the CPU driver's: verdict, state, piece table, text and the tail's model"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (S.STATUS[g["status"]], G.STATUS[g["gz_status"]]) == (w.status, w.gz_status), k
        assert g["window"] == (w.offset, w.len, w.bit, w.flags), k
        assert (g["consumed_bits"], g["text_len"], int(g["ended"])) == (w.consumed_bits, w.text_len, w.ended), k
        pieces, first = g["pieces"]
        assert first == [0, len(w.pieces)] and pieces == w.pieces, k
        assert g["member_status"] == [g["gz_status"]] and g["batch_len"] == len(g["carry_in"]) + text_cap + 1, k
        assert len(g["segments"]) == 1 and (g["segments"][0]["start"], g["segments"][0]["len"], g["segments"][0]["hits"]) == (0, g["batch_len"], g["n_hits"]), k
        if w.status != "OK":
            assert g["state"] is None and (g["carry"], g["bytes"], g["lines"], g["n_hits"], g["text_len"]) == (b"", 0, 0, 0, 0), k
            assert not with_text or g["batch"] == b"\n" * g["batch_len"], k
            continue
        st = g["state"]
        assert (st.text_bytes, st.crc, st.bit, st.history_bytes()) == (w.text_bytes, w.crc, w.state_bit, w.history), k
        full = g["carry_in"] + w.text
        nbytes, carry = model_tail(full, w.ended, CARRY_CAP)
        assert (g["bytes"], g["carry"], g["lines"]) == (nbytes, carry, full[:nbytes].count(b"\n")), k
        if with_text:
            assert g["batch"] == full[:nbytes] + b"\n" * (g["batch_len"] - nbytes), k


MODES = [FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_HITS | FETCH_COMPACT]


@pytest.mark.parametrize("name", ["v2_zblock", "v1_l6", "v4_seam", "v4_short_pieces"])
def test_chain(env, cpu, name):
    """text, consumed bits, states and piece tables equal the CPU driver's field for field; records in file coordinates, with line
    numbers that continue across windows, equal the plain scan's"""
    gz, text = S.vector(name)
    chain = S.CHAINS[name]
    want = cpu(gz, chain)
    S.check_chain(want, gz, text)
    got = run_chain(env, gz, chain, lines=True, fetch_mode=FETCH_SORTED)
    check_against_cpu(env, got, want, chain[2])
    assert b"".join(g["batch"][:g["bytes"]] for g in got) == text
    assert sum(g["bytes"] for g in got) == len(text) and sum(g["lines"] for g in got) == text.count(b"\n")
    want_hits, want_numbered, _, want_n = plain(env, text, True)
    assert sum(g["n_hits"] for g in got) == want_n > 100
    assert sorted(h for g in got for h in g["hits"]) == want_hits          # every record exactly once
    assert sorted(x for g in got for x in g["numbered"]) == want_numbered
    assert sum(1 for g in got[:-1] if g["carry"]) >= min(2, len(got) - 1)  # seams that fall inside a line


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lines", [False, True])
def test_fetch_modes(env, cpu, mode, lines):
    gz, text = S.vector("v4_seam")
    chain = S.CHAINS["v4_seam"]
    got = run_chain(env, gz, chain, lines=lines, fetch_mode=mode, want_text=mode != FETCH_COUNTS)
    check_against_cpu(env, got, cpu(gz, chain), chain[2], with_text=mode != FETCH_COUNTS)
    want_hits, want_numbered, _, want_n = plain(env, text, lines)
    assert sum(g["n_hits"] for g in got) == want_n > 50
    if mode & 1 and mode != FETCH_DEVICE:
        assert sorted(h for g in got for h in g["hits"]) == want_hits
        if lines:
            assert sorted(x for g in got for x in g["numbered"]) == want_numbered


EVERY = 5000


def seam_vector():
    """log lines in blocks of EVERY bytes of text, with F.NEEDLE laid across every multiple of EVERY: wherever a window's text ends, at a
    block end, the indicator and its line straddle the seam -> (file, text)"""
    src = P.lines(900, 77).split(b"\n")
    buf, k, i = bytearray(), 1, 0
    while k * EVERY < 150000:
        at = k * EVERY - 4                                  # the needle's first byte: four of its bytes in front of the seam
        while at - len(buf) > 400:
            buf += src[i] + b"\n"
            i += 1
        head = b"GET /seam/%d from " % k
        buf += head + b"x" * (at - len(buf) - len(head) - 1) + b" " + F.NEEDLE + b" done\n"
        k += 1
    text = bytes(buf)
    return G.gz_wrap(P.deflate_blocks(text, EVERY), text), text


def test_an_indicator_that_straddles_a_window_seam(env, cpu):
    gz, text = seam_vector()
    chain = (8 << 10, 1024, 24 << 10)
    want = cpu(gz, chain)
    S.check_chain(want, gz, text)
    seams, done = [], 0
    for w in want[:-1]:
        done += w.text_len
        seams.append(done)
    assert len(seams) >= 5
    for s in seams:                                            # on the CPU driver: every seam falls inside the indicator
        assert s % EVERY == 0 and text[s - 4:s - 4 + len(F.NEEDLE)] == F.NEEDLE and b"\n" not in text[s - 20:s + 5]
    got = run_chain(env, gz, chain, lines=True, fetch_mode=FETCH_SORTED)
    check_against_cpu(env, got, want, chain[2])
    want_hits, want_numbered, _, _ = plain(env, text, True)
    hits = sorted(h for g in got for h in g["hits"])
    assert hits == want_hits and sorted(x for g in got for x in g["numbered"]) == want_numbered
    for s in seams:
        assert len([h for h in hits if (h[0], h[1]) == (s - 4, s - 4 + len(F.NEEDLE))]) == 1
    assert all(g["carry"].endswith(F.NEEDLE[:4]) for g in got[:-1])


def test_hit_lines_and_rendered_records(env):
    """every window with hit lines and records rendered on the GPU: the NDJSON block equals the host renderer's on the same result, from
    the batch and from the hit lines alone; the line numbers continue across windows through line_base"""
    M = env.M
    gz, text = S.vector("v4_seam")
    chain = S.CHAINS["v4_seam"]
    sc = M.Scanner(env.db)
    base = [0]
    blocks = []

    def scan(blob, state, carry, text_cap, flags):
        sc.set_render(flags=M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE, source="seam.gz", line_base=base[0])
        r = sc.scan_gz_stream(blob, state=state, carry=carry, carry_cap=CARRY_CAP, text_cap=text_cap, first=bool(flags & 1), file_end=bool(flags & 2), want_text=True,
                              fetch_mode=FETCH_SORTED)
        want = r.ndjson_lines_text(r.gz_text(), source="seam.gz", line_base=base[0], with_input_line=True)
        assert r.rendered_ndjson() == want and want.count(b"\n") == r.n_hits
        assert r.ndjson_lines_text(None, source="seam.gz", line_base=base[0], with_input_line=True) == want
        blocks.append(want)
        base[0] += r.lines
        return r
    try:
        sc.set_hit_lines(True)
        got = run_chain(env, gz, chain, lines=True, fetch_mode=FETCH_SORTED, sc=sc, scan=scan)
        assert all(g["status"] == 0 for g in got) and got[-1]["ended"] and base[0] == text.count(b"\n")
        assert sum(b.count(b"\n") for b in blocks) == plain(env, text, True)[3] > 50 and all(b"seam.gz" in b for b in blocks if b)
    finally:
        sc.close()


def test_no_progress_and_failures(env, cpu):
    """v3_fixed has no block start to land on: NO_PROGRESS, the batch is all newlines, no hit, and the scanner goes on; a capacity below
    the first block; the preset dictionary; a header that does not parse; the trailer mutants fail in the last window only"""
    M = env.M
    fixed, _ = S.vector("v3_fixed")
    for gz, chain in ((fixed, (8 << 10, 1024, 1 << 20)), (S.vector("v2_zblock")[0], (16 << 10, 1024, 19999)), (S.vector("v6_dict_piece0")[0], (4 << 10, 512, 64 << 10)),
                      (S.vector("v6_dict_later")[0], (4 << 10, 512, 64 << 10)), (b"\x1f\x8c" + fixed[2:], (16 << 10, 1024, 48 << 10))):
        got = run_chain(env, gz, chain)
        check_against_cpu(env, got, cpu(gz, chain), chain[2])
        assert got[-1]["status"] != M.STREAM_OK and got[-1]["n_hits"] == 0 and got[-1]["batch"] == b"\n" * got[-1]["batch_len"]
    assert run_chain(env, fixed, (8 << 10, 1024, 1 << 20))[0]["status"] == M.STREAM_NO_PROGRESS
    for name in ("v2_zblock", "v4_seam"):
        for what, gz, status in S.trailer_mutants(name):
            got = run_chain(env, gz, S.CHAINS[name])
            want = cpu(gz, S.CHAINS[name])
            check_against_cpu(env, got, want, S.CHAINS[name][2])
            assert all(g["status"] == M.STREAM_OK for g in got[:-1]) and len(got) >= 5
            assert (got[-1]["status"], G.STATUS[got[-1]["gz_status"]]) == (M.STREAM_FAILED, status)
    # usable afterwards
    gz, text = S.vector("v4_short_pieces")
    got = run_chain(env, gz, S.CHAINS["v4_short_pieces"])
    assert b"".join(g["batch"][:g["bytes"]] for g in got) == text


def test_mutant_sample(env, cpu):
    """64 bit flips and prefixes of P.mutant_source(), a fixed sample: every window's verdict is the CPU driver's"""
    gz, _ = P.mutant_source()
    for i in P.mutant_sample(64, seed=9):
        m = P.mutant_at(gz, i)
        got = run_chain(env, m, S.MUTANT_CHAIN, want_text=False)
        check_against_cpu(env, got, cpu(m, S.MUTANT_CHAIN), S.MUTANT_CHAIN[2], with_text=False)


def test_parameter_errors_leave_the_scanner_usable(env):
    M = env.M
    L = M.lib()
    sc = M.Scanner(env.db, profile=True)
    try:
        gz, text = S.vector("v4_short_pieces")
        chain = S.CHAINS["v4_short_pieces"]
        raw = M._ScanResult()
        ok_state = M.GzStreamState(100, 0, 3, 50)

        def window(state=None, carry=None, carry_len=0, carry_cap=64, text_cap=4096, flags=M.STREAM_FIRST):
            return M._GzStreamWindow(C.pointer(state) if state is not None else None, carry, carry_len, carry_cap, text_cap, flags)
        w = window()
        assert L.matchy_scanner_scan_gz_stream(sc._h, gz, len(gz), C.byref(w), 1, False, C.byref(raw)) == -5 and "pieces" in M.last_error()   # pieces off
        sc.set_gz_pieces(512)
        for w, word in ((window(carry_len=65), "carry_cap"), (window(carry_len=3), "NULL"), (window(flags=4), "flag"), (window(flags=0), "state"),
                        (window(state=M.GzStreamState(100, 0, 8, 50), flags=0), "bit"), (window(state=M.GzStreamState(1 << 20, 0, 0, 32769), flags=0), "history_len"),
                        (window(state=M.GzStreamState(49, 0, 0, 50), flags=0), "history_len"), (window(text_cap=0), "text_cap"),
                        (window(text_cap=(1 << 31) - 1), "2^31"), (window(carry_cap=1 << 31), "2^31")):
            assert L.matchy_scanner_scan_gz_stream(sc._h, gz, len(gz), C.byref(w), 1, False, C.byref(raw)) == -5 and word in M.last_error(), word
        w = window(state=ok_state, flags=0)
        assert L.matchy_scanner_scan_gz_stream(sc._h, gz, 0, C.byref(w), 1, False, C.byref(raw)) == -5
        assert L.matchy_scanner_scan_gz_stream(sc._h, gz, len(gz), None, 1, False, C.byref(raw)) == -5
        assert L.matchy_scan_result_gz_stream(None, None, None, None, None, None, None, None, None) == -5
        sc.set_whole_lines(True)
        w = window()
        assert L.matchy_scanner_scan_gz_stream(sc._h, gz, len(gz), C.byref(w), 1, False, C.byref(raw)) == -5   # the whole-lines refusal
        sc.set_whole_lines(False)
        # ... and a plain scan and a window scan give, before and after a chain, what they gave
        def others():
            r = sc.scan(text[:20000])
            a = (keyed(r.hits()), r.n_hits, r.lines)
            assert r.gz_stream() is None
            r.close()
            r = sc.scan_gz_window(F.member(text[:9000]) + F.member(text[9000:20000]), carry=b"GET /c ", carry_cap=4096, want_text=True)
            b = (keyed(r.hits()), r.gz_window(), r.gz_text(), r.bytes, r.lines)
            assert r.gz_stream() is None
            r.close()
            return a, b
        before = others()
        got = run_chain(env, gz, chain, sc=sc)
        assert b"".join(g["batch"][:g["bytes"]] for g in got) == text and len(got) >= 5
        t = sc.gz_stream_timing_ms()
        assert list(t) == list(M.GZ_STREAM_PASSES) and all(v > 0 for v in t.values()), t
        assert others() == before
        assert all(v == 0 for v in sc.gz_stream_timing_ms().values())
    finally:
        sc.close()


def test_multi_scanner_returns_what_the_scanner_returns(env, cpu):
    """submit_gz_stream_ptr on one device: verdict, state, carry, text and records of every window of a chain equal the scanner's"""
    M = env.M
    gz, text = S.vector("v4_short_pieces")
    chain = S.CHAINS["v4_short_pieces"]
    want = run_chain(env, gz, chain, fetch_mode=FETCH_SORTED)
    ms = M.MultiScanner(env.db, devices=(0,))
    try:
        ms.set_gz_pieces(chain[1])
        state, carry = None, b""
        for k, g in enumerate(want):
            offset, length, _, flags = g["window"]
            keep = C.create_string_buffer(gz[offset:offset + length], length)
            ms.submit_gz_stream_ptr(C.addressof(keep), length, state=state, carry=carry, carry_cap=CARRY_CAP, text_cap=chain[2], first=bool(flags & 1), file_end=bool(flags & 2),
                                    want_text=True, tag=k)
            b = ms.next(want_hits=True)
            v = b["gz_stream"]
            assert (b["seq"], b["tag"]) == (k, k) and (v["status"], v["consumed_bits"], v["text_len"], v["ended"], v["carry"]) == (0, g["consumed_bits"], g["text_len"], g["ended"], g["carry"])
            same = lambda a, c: (a.text_bytes, a.crc, a.bit, a.history_bytes()) == (c.text_bytes, c.crc, c.bit, c.history_bytes())   # noqa: E731
            assert same(v["state"], g["state"]) and b["text"] == g["batch"] and b["n_hits"] == g["n_hits"] and keyed(b["hits"], g["shift"]) == g["hits"]
            state, carry = v["state"], v["carry"]
        assert ms.next() is None and want[-1]["ended"] and len(want) >= 5
    finally:
        ms.close()
