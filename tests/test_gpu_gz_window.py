"""GPU: gz windows (matchy_scanner_scan_gz_window; csrc/inflate.hip: k_gz_window_tail). A multi-member file is cut into windows of whole
members, the windows are scanned one after another and every window hands the bytes behind its last newline — the carry — to the next.
Expected text comes from zlib through gzip.decompress; expected records come from the existing path: the plain scan of the whole text on
a second scanner. A window's batch starts at the file offset of the bytes consumed so far (its carry is the file's bytes in front of its
members), so batch offsets map to file offsets by adding that count. The corrupt vector runs here only behind the sanitizer tests of the
decoder rules (tests/test_inflate_core_host.py, tests/test_gz_files_host.py)."""
import ctypes as C
import gzip
import zlib

import pytest

import gz_cases as G
import gz_files_cases as F
import gz_window_cases as W
import test_gpu_gz as T
import test_gpu_gz_files as TF

pytestmark = pytest.mark.gpu

FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_COMPACT = 0, 1, 3, 4, 8
BLOCK = 4096   # GZ_TAIL_BLOCK, pinned by tests/test_gz_window_host.py against csrc/inflate.h


@pytest.fixture(scope="module")
def env():
    e = T.Env()
    assert e.M.GZ_WINDOW_TAIL_BLOCK == BLOCK
    yield e
    e.sc.close(); e.ref.close(); e.db.close()


def keyed(hits, shift=0):
    return sorted((h["start"] + shift, h["end"] + shift, h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"], tuple(h["ids"])) for h in hits)


def numbered(r, shift=0, line_base=0):
    """[(hit start, line, line start, line end)] of a result scanned with line context, in file coordinates"""
    recs = list(r.ip4_lines or []) + list(r.line_records or [])
    return sorted((h["start"] + shift, ln + line_base, ls + shift, le + shift) for h, (ln, ls, le) in zip(r.hits(), recs))


def scan_window(sc, blob, carry=b"", carry_cap=4096, last=False, lines=False, fetch_mode=FETCH_HITS, want_text=True, shift=0, line_base=0):
    sc.set_line_context(lines)
    r = sc.scan_gz_window(blob, carry=carry, carry_cap=carry_cap, last=last, want_text=want_text, fetch_mode=fetch_mode)
    status, new_carry = r.gz_window()
    out = dict(status=status, carry=new_carry, text=r.gz_text(), text_len=r.gz_text_len(), bytes=r.bytes, lines=r.lines, n_hits=r.n_hits,
               file_status=r.gz_file_status(), first_member=r.gz_first_member(), member_status=r.gz_status(), segments=r.segments,
               hits=keyed(r.hits(), shift) if fetch_mode & 1 else None, numbered=numbered(r, shift, line_base) if lines and fetch_mode & 1 else None)
    r.close()
    return out


def plain(env, text, lines=False):
    env.ref.set_line_context(lines)
    r = env.ref.scan(text)
    out = keyed(r.hits()), (numbered(r) if lines else None), r.lines, r.n_hits
    r.close()
    return out


def run_chain(env, windows, carry_cap=4096, lines=False, fetch_mode=FETCH_HITS, sc=None):
    """scans the windows of one file in order, the carry fed forward, and holds every window against the model of the chain and the
    whole file against the plain scan of its text. Returns the per-window results."""
    sc = sc or env.sc
    texts = [gzip.decompress(w) for w in windows]
    text = b"".join(texts)
    model = W.chain(texts, carry_cap)
    assert len(model) == len(windows) and all(m[5] == 0 for m in model)
    got, carry, consumed, line_base = [], b"", 0, 0
    for k, (w, (carry_in, batch, carry_out, nbytes, nlines, _)) in enumerate(zip(windows, model)):
        assert carry == carry_in
        g = scan_window(sc, w, carry=carry, carry_cap=carry_cap, last=k + 1 == len(windows), lines=lines, fetch_mode=fetch_mode,
                        want_text=fetch_mode != FETCH_COUNTS, shift=consumed, line_base=line_base)
        assert g["status"] == 0 and g["file_status"] == [0] and g["first_member"] == [0, len(F.split_members(w))], k
        assert g["text_len"] == len(batch) and (g["text"] == batch if fetch_mode != FETCH_COUNTS else g["text"] is None), k
        assert g["carry"] == carry_out and (g["bytes"], g["lines"]) == (nbytes, nlines), k
        assert len(g["segments"]) == 1 and (g["segments"][0]["start"], g["segments"][0]["len"], g["segments"][0]["hits"]) == (0, len(batch), g["n_hits"]), k
        got.append(g)
        carry, consumed, line_base = g["carry"], consumed + g["bytes"], line_base + g["lines"]
    # each window's own text minus its tail, concatenated, is the file's text
    if fetch_mode != FETCH_COUNTS:
        assert b"".join(g["text"][:g["bytes"]] for g in got) == text
    assert sum(g["bytes"] for g in got) == len(text) and sum(g["lines"] for g in got) == text.count(b"\n")
    want_hits, want_numbered, _, want_n = plain(env, text, lines)
    assert sum(g["n_hits"] for g in got) == want_n
    if fetch_mode & 1:
        assert sorted(h for g in got for h in g["hits"]) == want_hits          # every record exactly once
        if lines:
            assert sorted(x for g in got for x in g["numbered"]) == want_numbered
    return got


def chain_files():
    """(name, file): a BGZF-style file cut at arbitrary bytes with the empty end block, and 40 members without final newlines"""
    bgzf = F.bgzf_file(G.log(70, seed=21), 997)
    forty = b"".join(F.member(G.log(2, seed=300 + k, final_newline=False), 1 + k % 9) for k in range(40))
    return [("bgzf", bgzf), ("forty", forty)]


@pytest.mark.parametrize("mode", [FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_HITS | FETCH_COMPACT])
@pytest.mark.parametrize("lines", [False, True])
def test_chain(env, mode, lines):
    """windows of about 2 KiB of text, the carry fed forward: text, records, (line, line start, line end), bytes and lines of the file"""
    for name, f in chain_files():
        windows = W.cut_windows(f, 2048)
        texts = [gzip.decompress(w) for w in windows]
        model = W.chain(texts, 4096)
        assert b"".join(windows) == f and len(windows) >= 4, name                  # preconditions, from the model alone
        assert sum(1 for m in model[:-1] if m[2]) >= 2, name                        # boundaries that fall mid-line
        got = run_chain(env, windows, lines=lines, fetch_mode=mode)
        assert sum(1 for g in got if g["carry"]) >= 2 and sum(g["n_hits"] for g in got) > 20


def test_a_needle_that_straddles_a_window_boundary(env):
    """the address is cut in two by the boundary between two windows: it is absent from the earlier window, whose tail was blanked, and
    found once in the later one, on the right line"""
    f, text, line = F.straddle_file()
    a, b = F.pieces(f)
    got = run_chain(env, [a, b], lines=True, fetch_mode=FETCH_SORTED)
    at = text.index(F.NEEDLE)
    assert got[0]["carry"] == gzip.decompress(a).rsplit(b"\n", 1)[1] and got[0]["carry"].endswith(b"192.0")
    assert not [h for h in got[0]["hits"] if h[0] <= at < h[1] or at <= h[0] < at + len(F.NEEDLE)]
    mine = [x for x in got[1]["numbered"] if x[0] == at]
    assert len(mine) == 1 and [h for h in got[1]["hits"] if (h[0], h[1]) == (at, at + len(F.NEEDLE))]
    _, want_numbered, _, _ = plain(env, text, True)
    assert mine[0] in want_numbered and F.NEEDLE in text[mine[0][2]:mine[0][3]] and text[:mine[0][2]].count(b"\n") == line - 1
    assert got[1]["text"].startswith(got[0]["carry"] + b".2.7 done\n")


def tail_bytes(n):
    return bytes(65 + i % 26 for i in range(n))


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_tail_lengths(env, n):
    """a final line of n bytes without its newline: the carry is those bytes, the blanked range is all newlines, and everything in front
    of it is scanned; once with a carry in front, once across two members"""
    head = G.log(6, seed=31)
    tail = tail_bytes(n)
    want_hits, _, _, want_n = plain(env, head)
    for carry_in, blobs in ((b"", [head + tail]), (b"GET /", [head[:100], head[100:] + tail[:n // 2], tail[n // 2:]])):
        blob = b"".join(F.member(x) for x in blobs)
        g = scan_window(env.sc, blob, carry=carry_in, carry_cap=2 * BLOCK + 1)
        assert g["status"] == 0 and g["file_status"] == [0]
        assert g["carry"] == tail and g["text"] == carry_in + head + b"\n" * n
        assert g["bytes"] == len(carry_in) + len(head) and g["lines"] == head.count(b"\n")
        if not carry_in:
            assert g["hits"] == want_hits and g["n_hits"] == want_n > 0
        assert all(h[1] <= len(carry_in) + len(head) for h in g["hits"])


def test_carry_cap(env):
    """a tail equal to the cap is carried; one byte more is NO_LINE_END: all newlines, no hit, no bytes. A window without any newline
    is carried whole up to the cap and NO_LINE_END above it"""
    M = env.M
    head = G.log(3, seed=32)
    needle_line = b"GET /x from " + F.NEEDLE + b" "
    for cap in (64, 100, 2048):
        tail = (needle_line + tail_bytes(cap))[:cap]
        g = scan_window(env.sc, F.member(head + tail), carry_cap=cap)
        assert (g["status"], g["carry"], g["bytes"], g["lines"]) == (M.WINDOW_OK, tail, len(head), head.count(b"\n"))
        assert g["text"] == head + b"\n" * cap and g["n_hits"] == plain(env, head)[3] > 0
        g = scan_window(env.sc, F.member(head + tail + b"z"), carry_cap=cap)
        assert (g["status"], g["carry"], g["bytes"], g["lines"], g["n_hits"]) == (M.WINDOW_NO_LINE_END, b"", 0, 0, 0)
        assert g["text"] == b"\n" * (len(head) + cap + 1) and g["file_status"] == [0]
        g = scan_window(env.sc, F.member(tail[cap // 2:]), carry=tail[:cap // 2], carry_cap=cap)      # no newline at all, carry + text == cap
        assert (g["status"], g["carry"], g["bytes"], g["lines"], g["n_hits"]) == (M.WINDOW_OK, tail, 0, 0, 0) and g["text"] == b"\n" * cap
        g = scan_window(env.sc, F.member(tail[cap // 2:] + b"z"), carry=tail[:cap // 2], carry_cap=cap)  # the same, one byte above the cap
        assert (g["status"], g["carry"], g["bytes"], g["lines"], g["n_hits"]) == (M.WINDOW_NO_LINE_END, b"", 0, 0, 0) and g["text"] == b"\n" * (cap + 1)
    assert F.NEEDLE in tail
    g = scan_window(env.sc, F.member(b"\n" + tail), carry_cap=2048)                # a newline as the window's first byte, the rest is tail
    assert (g["status"], g["carry"], g["bytes"], g["lines"]) == (M.WINDOW_OK, tail, 1, 1)
    g = scan_window(env.sc, F.member(head), carry_cap=0)                           # a window that ends in a newline needs no room
    assert (g["status"], g["carry"], g["bytes"], g["text"]) == (M.WINDOW_OK, b"", len(head), head)


def test_last_window(env):
    """the file ends here: nothing is cut, the last partial line is scanned, one separator, an empty carry; an empty last window with an
    empty carry has no separator and no text"""
    text = G.log(4, seed=33) + b"GET /last from " + F.NEEDLE
    g = scan_window(env.sc, F.member(text[:150]) + F.member(text[150:]), last=True, lines=True)
    want_hits, want_numbered, _, want_n = plain(env, text, True)
    assert (g["status"], g["carry"], g["bytes"], g["lines"]) == (0, b"", len(text), text.count(b"\n"))
    assert g["text"] == text + b"\n" and g["hits"] == want_hits and g["numbered"] == want_numbered and g["n_hits"] == want_n
    assert any(h[0] == len(text) - len(F.NEEDLE) for h in g["hits"])
    g = scan_window(env.sc, F.member(b"") + F.BGZF_EOF, last=True)
    assert (g["status"], g["carry"], g["bytes"], g["lines"], g["n_hits"], g["text_len"]) == (0, b"", 0, 0, 0, 0) and not g["text"]
    carry = b"GET /carried from " + F.NEEDLE
    g = scan_window(env.sc, F.BGZF_EOF, carry=carry, last=True)                    # only the carry: its line ends at the separator
    assert (g["status"], g["carry"], g["bytes"], g["lines"], g["text"]) == (0, b"", len(carry), 0, carry + b"\n")
    assert g["hits"] == plain(env, carry)[0] and g["n_hits"] == 1


@pytest.mark.parametrize("last", [False, True])
def test_failed_window(env, last):
    """one member with a flipped CRC bit: the file status is that member's, the whole batch — the carry-in with its needle included —
    is newlines, nothing is reported, nothing is carried"""
    M = env.M
    t = [G.log(2, seed=34), G.log(3, seed=35), G.log(2, seed=36) + b"partial"]
    bad = G.gz_wrap(G.raw_deflate(t[1]), t[1], crc=zlib.crc32(t[1]) ^ 0x100)
    carry = b"GET /c from " + F.NEEDLE + b" then"
    g = scan_window(env.sc, F.member(t[0]) + bad + F.member(t[2]), carry=carry, last=last, lines=True)
    n = len(carry) + sum(map(len, t))
    assert g["file_status"] == [M.GZ_CRC_MISMATCH] and g["member_status"] == [0, M.GZ_CRC_MISMATCH, 0]
    assert (g["status"], g["carry"], g["bytes"], g["lines"], g["n_hits"], g["hits"]) == (M.WINDOW_OK, b"", 0, 0, 0, [])
    assert g["text"] == b"\n" * (n + (1 if last else 0))
    good = scan_window(env.sc, F.member(t[0]) + F.member(t[1]) + F.member(t[2]), carry=carry, last=last)   # the same window, intact
    assert good["n_hits"] > 0 and good["carry"] == (b"" if last else b"partial") and any(h[0] == carry.index(F.NEEDLE) for h in good["hits"])


def test_multi_scanner_returns_what_the_scanner_returns(env):
    """submit_gz_window on one device: text, carry, status, verdict and records of every window of a chain equal the scanner's"""
    M = env.M
    windows = W.cut_windows(chain_files()[0][1], 2048)
    want = run_chain(env, windows, fetch_mode=FETCH_SORTED)
    ms = M.MultiScanner(env.db, devices=(0,))
    try:
        carry = b""
        for k, (w, g) in enumerate(zip(windows, want)):
            keep = C.create_string_buffer(w, len(w))
            ms.submit_gz_window_ptr(C.addressof(keep), len(w), carry=carry, carry_cap=4096, last=k + 1 == len(windows), want_text=True, tag=k)
            b = ms.next(want_hits=True)
            assert (b["seq"], b["tag"]) == (k, k) and b["window_status"] == g["status"] == 0 and b["carry"] == g["carry"]
            assert b["text"] == g["text"] and b["nbytes"] == g["text_len"] and b["gz_file_status"] == [0] and b["gz_status"] == g["member_status"]
            assert b["n_hits"] == g["n_hits"] and len(b["segments"]) == 1
            shift = sum(x["bytes"] for x in want[:k])
            assert keyed(b["hits"], shift) == g["hits"]
            carry = b["carry"]
        assert ms.next() is None
    finally:
        ms.close()


def test_the_other_gz_scans_are_untouched_by_a_window_scan(env):
    """scan_gz_files and scan_gz on the same scanner before and after window scans give what they gave; refused windows leave the
    scanner usable"""
    M = env.M
    L = M.lib()
    sc = M.Scanner(env.db)
    try:
        good, rej = F.good_files(), F.reject_files()
        files = [(f, t) for _, f, t in good[:4]] + [(rej[0][1], None)]
        before = TF.check_files(env, files, lines=True, sc=sc)
        pack = [(good[6][1], len(good[6][2]), good[6][2])]
        before_pack = T.check_pack(env, pack, sc=sc)
        run_chain(env, W.cut_windows(chain_files()[1][1], 2048), lines=True, sc=sc)
        raw = M._ScanResult()
        blob = good[0][1]
        for w, word in ((M._GzWindow(None, 65, 64, 0), "carry_cap"), (M._GzWindow(None, 3, 64, 0), "NULL"), (M._GzWindow(None, 0, 64, 4), "flag")):
            assert L.matchy_scanner_scan_gz_window(sc._h, blob, len(blob), C.byref(w), 1, False, C.byref(raw)) == -5 and word in M.last_error()
        w = M._GzWindow(None, 0, 64, 0)
        assert L.matchy_scanner_scan_gz_window(sc._h, blob, 0, C.byref(w), 1, False, C.byref(raw)) == -5
        sc.set_whole_lines(True)
        assert L.matchy_scanner_scan_gz_window(sc._h, blob, len(blob), C.byref(w), 1, False, C.byref(raw)) == -5   # the whole-lines refusal
        sc.set_whole_lines(False)
        assert TF.check_files(env, files, lines=True, sc=sc) == before
        assert T.check_pack(env, pack, sc=sc) == before_pack
        r = sc.scan_gz_files([good[0][1]])
        assert r.gz_window() is None
        r.close()
        run_chain(env, W.cut_windows(chain_files()[0][1], 2048), sc=sc)
    finally:
        sc.close()
