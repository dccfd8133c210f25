"""GPU: gz scans of multi-member files (matchy_scanner_scan_gz_files; csrc/inflate.hip: k_gz_file_verdict, k_gz_seal_files). Expected text
comes from zlib through gzip.decompress; expected records come from the existing path: the plain segmented scan of the same text laid
out by the model of the plan (gz_files_cases.layout_files) on a second scanner. The corrupt vectors run here only behind
tests/test_gz_files_host.py and tests/test_inflate_core_host.py, which drive the same host and decoder rules under a sanitizer."""
import ctypes as C
import gzip
import json

import numpy as np
import pytest

import gz_cases as G
import gz_files_cases as F
import test_gpu_gz as T

pytestmark = pytest.mark.gpu

FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_COMPACT = 0, 1, 3, 4, 8


@pytest.fixture(scope="module")
def env():
    e = T.Env()
    yield e
    e.sc.close(); e.ref.close(); e.db.close()


gzip_text = gzip.decompress


def first_bad(status, first, f):
    """the status a file must have: OK, or that of its first member in stream order that is not"""
    return next((s for s in status[first[f]:first[f + 1]] if s), 0)


def numbered(r):
    """[(hit start, (line, line start, line end))] of a result scanned with line context"""
    return list(zip([h["start"] for h in r.hits()], list(r.ip4_lines or []) + list(r.line_records or [])))


def check_files(env, files, lines=False, fetch_mode=FETCH_HITS, sc=None):
    """files: [(gzip file, expected text or None for a file that must fail)]. Scans the pack with want_text and holds verdicts, member
    table, text, records, segment indices, the segment table and the counters against the expected batch. Returns (file statuses, n_hits)."""
    sc = sc or env.sc
    caps = [(F.file_cap(b), t) for b, t in files]
    starts, batch = F.layout_files(caps)
    sc.set_line_context(lines)
    r = sc.scan_gz_files([b for b, _ in files], want_text=True, fetch_mode=fetch_mode)
    fs, first, ms = r.gz_file_status(), r.gz_first_member(), r.gz_status()
    assert len(fs) == len(files) and first[0] == 0 and first[-1] == len(ms)
    assert [b - a for a, b in zip(first, first[1:])] == [len(F.split_members(b)) for b, _ in files]
    assert fs == [first_bad(ms, first, f) for f in range(len(files))]
    assert [s == 0 for s in fs] == [t is not None for _, t in files], [G.STATUS[s] for s in fs]
    text = r.gz_text()
    assert r.gz_text_len() == len(batch)
    if text != batch:
        bad = [i for i, s in enumerate(starts) if text[s:s + caps[i][0] + 1] != batch[s:s + caps[i][0] + 1]]
        raise AssertionError(f"text differs from the expected batch, first in file {bad[:1]} of {len(files)} (lengths {len(text)}, {len(batch)})")
    want_recs, want_table, want_lines = T.reference(env, starts, batch, lines)
    assert T.table(r) == want_table and [s["start"] for s in r.segments] == starts
    if fetch_mode & 1:
        assert np.array_equal(T.records(r), want_recs)
    assert r.n_hits == len(want_recs)
    if lines and fetch_mode & 1:   # (line, line start, line end) of every hit, against the plain segmented scan
        env.ref.set_segments(starts)
        want = env.ref.scan(batch)
        assert sorted(numbered(r)) == sorted(numbered(want)) and len(numbered(r)) == r.n_hits
        want.close()
    ok = [t for _, t in files if t is not None]
    assert r.bytes == sum(len(t) for t in ok)
    assert r.lines == sum(t.count(b"\n") for t in ok)          # the inputs' own '\n' count
    assert want_lines - r.lines == sum(1 if t is not None else c + 1 for c, t in caps if c)
    n = r.n_hits
    r.close()
    return fs, n


@pytest.mark.parametrize("lines", [False, True])
def test_good_files(env, lines):
    """one pack of files of 2, 3 and 130 members, a BGZF-style file cut mid-line with the empty end block, empty members first / middle /
    last, only empty members, a single member, a one-byte member, later headers with every optional field"""
    good = F.good_files()
    fs, n = check_files(env, [(f, t) for _, f, t in good], lines=lines)
    assert fs == [0] * len(good) and n > 150


def test_a_needle_that_straddles_a_member_boundary(env):
    """the address is cut in two by the boundary between two members: it is found, on the right line of its file"""
    f, text, line = F.straddle_file()
    pad = F.member(G.log(4, seed=55))
    env.sc.set_line_context(True)
    r = env.sc.scan_gz_files([pad, f, pad], want_text=True, fetch_mode=FETCH_SORTED)
    batch = r.gz_text()
    assert r.gz_file_status() == [0, 0, 0] and r.gz_first_member() == [0, 1, 3, 4]
    out = r.ndjson_segments_text(batch, ["a.gz", "straddle.gz", "c.gz"], line_bases=[0, 0, 0])
    recs = [json.loads(ln) for ln in out.splitlines()]
    at = len(gzip_text(pad)) + 1 + text.index(F.NEEDLE)
    assert batch[at:at + len(F.NEEDLE)] == F.NEEDLE
    mine = [x for x in recs if x["source"] == "straddle.gz" and x["line_number"] == line]
    assert any(F.NEEDLE.decode() in json.dumps(x) for x in mine), mine
    assert any(h["start"] == at and h["end"] == at + len(F.NEEDLE) for h in r.hits())
    r.close()
    env.sc.set_line_context(False)


def test_rejects(env):
    """every reject between two good files in one pack: the verdict is the status of the first failing member in stream order, the whole
    file region is newlines — no hit from the good members of a failed file, whose first member holds a needle — and the neighbours are
    untouched"""
    rej, good = F.reject_files(), F.good_files()
    files, want = [(good[0][1], good[0][2])], [0]
    for k, (name, f, status) in enumerate(rej):
        files.append((f, None)); want.append(G.STATUS.index(status))
        g = good[1 + k % 4]
        files.append((g[1], g[2])); want.append(0)
    assert F.NEEDLE in gzip_text(F.pieces(rej[0][1])[0])
    fs, n = check_files(env, files, lines=True)
    assert [G.STATUS[s] for s in fs] == [G.STATUS[s] for s in want] and n > 0


def test_mutants(env):
    """every single-bit flip of a three-member file of about 600 compressed bytes, none skipped: the GPU saying OK implies that zlib
    accepts and the text is identical; zlib refusing implies that the GPU does not say OK. A flip in an ISIZE field can vouch for up
    to 4 GiB of text: a mutant whose pieces vouch for 4 MiB or more is scanned alone (the plan may refuse it: that is not OK either),
    the others share one pack with a pristine copy after every sixteenth."""
    src, text = F.mutant_source()
    assert 500 < len(src) < 700 and len(F.split_members(src)) == 3
    fs, _ = check_files(env, [(src, text)])
    assert fs == [0]
    muts = list(F.all_bit_flips(src))
    assert len(muts) == 8 * len(src)
    pack, alone = [], []
    for m in muts:
        (alone if F.file_cap(m) >= 1 << 22 else pack).append(m)
    assert len(alone) < 64 and len(pack) > 4000
    files = []
    for k, m in enumerate(pack):
        files.append(m)
        if k % 16 == 15:
            files.append(src)
    files.append(src)
    r = env.sc.scan_gz_files(files, want_text=True)
    fs, batch, starts = r.gz_file_status(), r.gz_text(), [s["start"] for s in r.segments]
    r.close()
    n_ok = 0
    for b, st, at in zip(files, fs, starts):
        accepted, t = F.zlib_accepts(b)
        if st == 0:
            assert accepted and batch[at:at + len(t)] == t and F.file_cap(b) == len(t)
            n_ok += 1
        else:
            cap = F.file_cap(b)
            assert batch[at:at + cap] == b"\n" * cap
        if not accepted:
            assert st != 0
        if b is src:
            assert st == 0
    assert n_ok > len(files) // 17
    for m in alone:
        accepted, t = F.zlib_accepts(m)
        try:
            r = env.sc.scan_gz_files([m], want_text=False, fetch_mode=FETCH_COUNTS)
            st = r.gz_file_status()[0]
            r.close()
        except RuntimeError as e:
            assert "2^31" in str(e) or "too large" in str(e)
            st = -1
        assert st != 0 and not accepted   # a capacity of 4 MiB for 600 bytes: the ISIZE is wrong, and zlib says so too
    fs, _ = check_files(env, [(src, text)])
    assert fs == [0]


@pytest.mark.parametrize("mode", [FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_HITS | FETCH_COMPACT])
def test_fetch_modes_and_tally(env, mode):
    """every fetch mode on a pack with one failed file, with the tally on: counts per value equal those of the segmented reference scan"""
    M = env.M
    good, rej = F.good_files(), F.reject_files()
    files = [(f, t) for _, f, t in good[:4]] + [(rej[0][1], None)] + [(f, t) for _, f, t in good[4:]]
    starts, batch = F.layout_files([(F.file_cap(b), t) for b, t in files])
    a, b = M.Scanner(env.db), M.Scanner(env.db)
    try:
        a.set_tally(True); b.set_tally(True)
        r = a.scan_gz_files([f for f, _ in files], want_text=mode != FETCH_COUNTS, fetch_mode=mode)
        b.set_segments(starts)
        want = b.scan(batch)
        assert r.n_hits == want.n_hits and T.table(r) == T.table(want) and r.n_hits > 150
        assert r.on_device == (mode == FETCH_DEVICE)
        assert [s == 0 for s in r.gz_file_status()] == [t is not None for _, t in files]
        assert (r.gz_text() == batch) if mode != FETCH_COUNTS else (r.gz_text() is None and r.gz_text_len() == len(batch))
        if mode & 1:
            assert np.array_equal(T.records(r), T.records(want))
        if mode == FETCH_HITS | FETCH_COMPACT:
            assert r.n_ip4_hits > 0
        if mode == FETCH_SORTED:
            assert r.hits() == want.hits() and r.segment_of == want.segment_of
        ta, tb = a.tally(), b.tally()
        assert list(ta) == list(tb) and (ta.distinct, ta.matches) == (tb.distinct, tb.matches) and ta.matches == r.n_hits
        r.close(); want.close()
    finally:
        a.close(); b.close()


def test_hit_lines_and_rendered_records(env):
    """hit lines and records rendered on the GPU on a pack with one failed file: the NDJSON block equals the host renderer's"""
    M = env.M
    good, rej = F.good_files(), F.reject_files()
    files = [(f, t) for _, f, t in good[:3]] + [(rej[0][1], None)] + [(f, t) for _, f, t in good[3:6]]
    sources = ["in%d.gz" % k for k in range(len(files))]
    sc = M.Scanner(env.db)
    try:
        sc.set_hit_lines(True)
        flags = M.RENDER_LINE_NUMBERS | M.RENDER_INPUT_LINE
        sc.set_render(flags=flags, sources=sources, line_bases=[0] * len(files))
        r = sc.scan_gz_files([f for f, _ in files], want_text=True, fetch_mode=FETCH_SORTED)
        assert [s == 0 for s in r.gz_file_status()] == [t is not None for _, t in files]
        batch = r.gz_text()
        want = r.ndjson_segments_text(batch, sources, line_bases=[0] * len(files), with_input_line=True)
        assert r.rendered_ndjson() == want and want.count(b"\n") == r.n_hits and r.n_hits > 50
        assert r.ndjson_segments_text(None, sources, line_bases=[0] * len(files), with_input_line=True) == want   # from the hit lines alone
        assert b"in3.gz" not in want
        r.close()
    finally:
        sc.close()


def test_buffers_are_reused_and_the_old_entries_are_untouched(env):
    """three packs of different shapes on one scanner, with a matchy_scanner_scan_gz call and a plain scan in between that give what
    they gave before; a two-member file through the OLD entry still reports TRAILING_DATA"""
    M = env.M
    sc = M.Scanner(env.db)
    try:
        good, rej = F.good_files(), F.reject_files()
        x = G.log(3, seed=66)
        two = F.member(x) * 2   # members of one length: the stream of the first ends at the capacity the old entry reads from the file's end
        fs, _ = check_files(env, [(f, t) for _, f, t in good], sc=sc)
        assert fs == [0] * len(good)
        r = sc.scan_gz([two, good[6][1]], want_text=True)
        assert r.gz_status() == [M.GZ_TRAILING_DATA, 0] and r.gz_file_status() is None and r.gz_first_member() is None
        assert r.gz_text() == b"\n" * (len(x) + 1) + good[6][2] + b"\n"
        r.close()
        fs, _ = check_files(env, [(good[6][1], good[6][2]), (rej[4][1], None)], sc=sc, lines=True)
        assert fs == [0, M.GZ_TRAILING_DATA]
        T.check_pack(env, [(good[6][1], len(good[6][2]), good[6][2])], sc=sc)
        plain = G.log(200, seed=13)
        a, b = sc.scan(plain), env.ref.scan(plain)
        assert a.hits() == b.hits() and (a.lines, a.bytes, a.candidates) == (b.lines, b.bytes, b.candidates) and a.n_hits > 100
        assert a.gz_status() is None and a.gz_file_status() is None and not a.has_segments
        a.close(); b.close()
        fs, _ = check_files(env, [(f, t) for _, f, t in good[2:5]] * 3, sc=sc)
        assert fs == [0] * 9
    finally:
        sc.close()


def test_bad_tables_leave_the_scanner_usable(env):
    M = env.M
    L = M.lib()
    f = F.good_files()[0][1]
    raw = M._ScanResult()
    table = (M._GzFile * 1)()
    for offset, length, n in ((len(f) + 1, 0, 1), (1, len(f), 1), (0, len(f), 0), (0, 1 << 32, 1)):
        table[0].offset, table[0].len = offset, length
        assert L.matchy_scanner_scan_gz_files(env.sc._h, f, len(f), table, n, 1, False, C.byref(raw)) == -5
        assert M.last_error()
    env.sc.set_whole_lines(True)
    table[0].offset, table[0].len = 0, len(f)
    assert L.matchy_scanner_scan_gz_files(env.sc._h, f, len(f), table, 1, 1, False, C.byref(raw)) == -5   # the whole-lines refusal
    env.sc.set_whole_lines(False)
    fs, _ = check_files(env, [(f, F.good_files()[0][2])])
    assert fs == [0]


def test_unix_header_patterns_are_refused_and_the_scanner_stays_usable(env):
    """1 000 bare headers with OS 3: 500 pieces of 20 bytes whose last four bytes vouch for 48 MiB each. The plan refuses the batch at
    2^31 bytes — alone and with good neighbours — with MATCHY_ERROR_INVALID_PARAM, and the next scan is what it always was"""
    M = env.M
    L = M.lib()
    good = F.good_files()
    for blobs in ([F.header_patterns(os_byte=3)], [good[0][1], F.header_patterns(os_byte=3), good[1][1]]):
        packed, table = M._gz_pack_files(blobs)
        raw = M._ScanResult()
        assert L.matchy_scanner_scan_gz_files(env.sc._h, packed, len(packed), table, len(table), 1, True, C.byref(raw)) == -5
        assert "2^31" in M.last_error() and not raw.n_hits
    fs, n = check_files(env, [(good[0][1], good[0][2]), (F.header_patterns(), None), (good[1][1], good[1][2])])
    assert fs == [0, M.GZ_BAD_BLOCK, 0] and n > 0


def test_multi_scanner_in_submission_order(env):
    """two workers on one device: packs of files come back in submission order with verdicts, member table, text and records"""
    M = env.M
    ms = M.MultiScanner(env.db, devices=(0, 0))
    try:
        good, rej = F.good_files(), F.reject_files()
        packs, keep = [], []
        for k in range(5):
            files = [(f, t) for _, f, t in good[k:k + 3]]
            if k == 3:
                files.insert(1, (rej[0][1], None))
            packed = C.create_string_buffer(b"".join(f for f, _ in files), sum(len(f) for f, _ in files))
            keep.append(packed)
            table_, pos = [], 0
            for f, _ in files:
                table_.append((pos, len(f)))
                pos += len(f)
            packs.append(files)
            ms.submit_gz_files_ptr(C.addressof(packed), len(packed.raw), table_, want_text=k != 2, tag=k)
            if ms.pending() >= ms.max_pending():
                pytest.fail("five batches fit the in-flight bound of two workers")
        for k, files in enumerate(packs):
            b = ms.next(want_hits=True)
            starts, batch = F.layout_files([(F.file_cap(f), t) for f, t in files])
            assert (b["seq"], b["tag"]) == (k, k)
            assert [s == 0 for s in b["gz_file_status"]] == [t is not None for _, t in files]
            assert b["gz_first_member"][-1] == len(b["gz_status"]) == sum(len(F.split_members(f)) for f, _ in files)
            assert b["nbytes"] == len(batch) and b["text"] == (batch if k != 2 else None)
            want_recs, want_table, _ = T.reference(env, starts, batch, False)
            assert [tuple(s.values()) for s in b["segments"]] == want_table
            assert sorted(h["start"] for h in b["hits"]) == sorted(want_recs[:, 0].tolist())
        assert ms.next() is None
    finally:
        ms.close()
