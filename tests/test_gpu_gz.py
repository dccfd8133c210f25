"""GPU: gz scans (matchy_scanner_scan_gz, csrc/inflate.hip). Expected bytes come from Python's zlib; expected hits come from the existing
path: matchy_scanner_scan with set_segments over the same text inflated on the host and laid out by the same plan (gz_cases.layout).
The corrupt vectors run here only behind tests/test_inflate_core_host.py, which drives the same decoder rules under a sanitizer."""
import ctypes as C

import numpy as np
import pytest

import gz_cases as G

pytestmark = pytest.mark.gpu

HIT = np.dtype([("start", "<u4"), ("len_type", "<u4"), ("value", "<u4"), ("kind", "u1"), ("prefix_len", "u1"), ("n_ids", "<u2")])
FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_COMPACT = 0, 1, 3, 4, 8


class Env:
    def __init__(self):
        import matchy_amd as M
        self.M = M
        self.db = M.Database(G.blob())
        self.sc = M.Scanner(self.db)      # gz scans
        self.ref = M.Scanner(self.db)     # the reference: segmented scans of host-inflated text


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.sc.close(); e.ref.close(); e.db.close()


def u32(ptr, n):
    return np.frombuffer(C.string_at(ptr, 4 * n), dtype="<u4") if ptr and n else np.zeros(0, dtype="<u4")


def records(r):
    """the hits of a host-resident result as sorted rows (start, len_type, kind, prefix_len, segment): compact records expanded"""
    raw = r._raw
    sa = r._segment_arrays()
    rows = []
    if raw.ip4_hits and raw.n_ip4_hits:
        c = np.frombuffer(C.string_at(C.cast(raw.ip4_hits, C.c_void_p).value, 8 * raw.n_ip4_hits), dtype="<u4").reshape(-1, 2)
        packed = c[:, 1].astype(np.int64)
        rows.append(np.stack([c[:, 0].astype(np.int64), ((packed >> 22) & 15) + 7 | 2 << 24, np.full(len(c), 2), packed >> 26,
                              u32(sa[1], raw.n_ip4_hits).astype(np.int64)], axis=1))
    if raw.hits and raw.n_hits:
        h = np.frombuffer(C.string_at(C.cast(raw.hits, C.c_void_p).value, 16 * raw.n_hits), dtype=HIT)
        rows.append(np.stack([h["start"].astype(np.int64), h["len_type"].astype(np.int64), h["kind"].astype(np.int64), h["prefix_len"].astype(np.int64),
                              u32(sa[0], raw.n_hits).astype(np.int64)], axis=1))
    if not rows:
        return np.zeros((0, 5), dtype=np.int64)
    a = np.concatenate(rows)
    return a[np.lexsort(a.T[::-1])]


def table(r):
    return [tuple(s.values()) for s in r.segments]


def reference(env, starts, batch, lines):
    """(records, table, result.lines) of the segmented scan of the expected batch"""
    env.ref.set_line_context(lines)
    env.ref.set_segments(starts)
    r = env.ref.scan(batch)
    out = records(r), table(r), r.lines
    r.close()
    return out


def check_pack(env, members, lines=False, fetch_mode=FETCH_HITS, use_out_lens=True, sc=None):
    """members: [(gz, out_len, expected text or None for a member that must fail)]. Scans the pack with want_text and holds statuses,
    text, records, segment indices, the table and the counters against the expected batch. Returns (result statuses, n_hits)."""
    sc = sc or env.sc
    caps = [(G.plan_status_cap(gz, out_len)[1], t) for gz, out_len, t in members]
    starts, batch = G.layout(caps)
    sc.set_line_context(lines)
    r = sc.scan_gz([gz for gz, _, _ in members], want_text=True, out_lens=[o for _, o, _ in members] if use_out_lens else None, fetch_mode=fetch_mode)
    status = r.gz_status()
    assert [s == 0 for s in status] == [t is not None for _, _, t in members]
    text = r.gz_text()
    assert r.gz_text_len() == len(batch)
    if text != batch:   # name the first member that differs instead of printing megabytes
        bad = [i for i, s in enumerate(starts) if text[s:s + caps[i][0] + 1] != batch[s:s + caps[i][0] + 1]]
        raise AssertionError(f"text differs from the expected batch, first in member {bad[:1]} of {len(members)} (lengths {len(text)}, {len(batch)})")
    want_recs, want_table, want_lines = reference(env, starts, batch, lines)
    assert table(r) == want_table
    if fetch_mode & 1:
        assert np.array_equal(records(r), want_recs)
    assert r.n_hits == len(want_recs)
    ok = [t for _, _, t in members if t is not None]
    assert r.bytes == sum(len(t) for t in ok)
    assert r.lines == sum(t.count(b"\n") for t in ok)
    assert want_lines - r.lines == sum(1 if t is not None else c + 1 for c, t in caps if c)   # separators and overwritten regions
    n = r.n_hits
    print(f"pack of {len(members)}: {sum(1 for s in status if s)} failed, {len(batch)} bytes of text, {n} hits")
    r.close()
    return status, n


@pytest.mark.parametrize("lines", [False, True])
def test_good_streams(env, lines):
    """(a) and (b) as one pack: the text is the plan's layout of zlib's outputs byte for byte, separators included; hits, segment_of and
    the per-segment table equal the segmented scan of the host-inflated pack"""
    cases = G.good_cases()
    status, n = check_pack(env, [(gz, out_len, text) for _, gz, out_len, _, text in cases], lines=lines)
    assert status == [0] * len(cases) and n > 1000


def test_good_streams_with_isize_as_capacity(env):
    """out_len 0 for every member: the capacity comes from the trailers"""
    cases = G.good_cases()
    members = [(gz, len(text), text) for _, gz, _, _, text in cases]
    status, _ = check_pack(env, members, use_out_lens=False)
    assert status == [0] * len(cases)


def test_rejects(env):
    """(c): the status of every rule, the whole region of a failed member is newlines, its good neighbours are intact, and the hits are
    those of the pack with the failed members' text replaced by newlines. The back-reference in front of the batch comes first."""
    rej, good = G.reject_cases(), G.good_cases()
    assert rej[0][0] == "dist1_at_0"
    members, want = [], []
    for k, (name, gz, out_len, status, _) in enumerate(rej):
        members.append((gz, out_len, None)); want.append(G.STATUS.index(status))
        g = good[2 + k % 3]
        members.append((g[1], g[2], g[4])); want.append(0)
    status, n = check_pack(env, members, lines=True)
    assert status == want and n > 0


@pytest.mark.parametrize("which", [0, 1])
def test_mutants(env, which):
    """(d): every single-bit flip of body and trailer and every proper prefix, each beside a pristine copy: zlib decides. A member zlib
    rejects, or does not see the end of, has a status other than OK and a region of newlines; one it accepts is OK and byte-equal. The
    pristine neighbours are compared byte for byte, so a wave that writes outside its member is seen."""
    name, gz, text = G.mutant_sources()[which]
    flips = list(G.bit_flips(gz))
    late = sum(1 for m in flips for ok, _, produced in [G.zlib_verdict(m)] if not ok and produced)
    assert late * 2 >= len(flips)
    pack = G.mutant_pack(gz, text, flips + list(G.prefixes(gz)))
    assert pack[-1][0] == gz and all(m[0] == gz for m in pack[1::2])
    status, n = check_pack(env, [(m, out_len, t) for m, out_len, _, t in pack])
    assert sum(1 for s in status if s) >= len(flips) - 16 and n > 0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 5000])
def test_pack_sizes(env, n):
    """resident waves outnumber the members, and the members outnumber the resident waves"""
    texts = [G.log(1 + i % 5, seed=i + 1, final_newline=i % 7 != 0) for i in range(min(n, 50))]
    files = [G.gz_wrap(G.raw_deflate(t, 1 + i % 9), t) for i, t in enumerate(texts)]
    members = [(files[i % len(files)], len(texts[i % len(files)]), texts[i % len(files)]) for i in range(n)]
    status, _ = check_pack(env, members, lines=n == 65)
    assert status == [0] * n


def test_buffers_are_reused_and_plain_scans_are_untouched(env):
    """two packs in a row on one scanner, the second smaller; then an ordinary scan on that scanner returns what a fresh scanner returns"""
    M = env.M
    sc = M.Scanner(env.db)
    try:
        big, small = G.log(300, seed=11), G.log(5, seed=12)
        for texts in ([big, small, big, b"", small] * 20, [small, big]):
            members = [(G.gz_wrap(G.raw_deflate(t), t), len(t), t) for t in texts]
            status, _ = check_pack(env, members, sc=sc)
            assert status == [0] * len(texts)
        plain = G.log(200, seed=13)
        a, b = sc.scan(plain), env.ref.scan(plain)
        assert a.hits() == b.hits() and (a.lines, a.bytes, a.candidates) == (b.lines, b.bytes, b.candidates) and a.n_hits > 100
        assert a.gz_status() is None and not a.has_segments
        a.close(); b.close()
    finally:
        sc.close()


@pytest.mark.parametrize("mode", [FETCH_COUNTS, FETCH_HITS, FETCH_SORTED, FETCH_DEVICE, FETCH_HITS | FETCH_COMPACT])
def test_fetch_modes_and_tally(env, mode):
    """every fetch mode, with the tally on: counts per value equal those of the segmented reference scan"""
    M = env.M
    rej, good = G.reject_cases(), G.good_cases()
    members = [(g[1], g[2], g[4]) for g in good[2:9]] + [(rej[1][1], rej[1][2], None)] + [(g[1], g[2], g[4]) for g in good[9:]]
    caps = [(G.plan_status_cap(gz, out_len)[1], t) for gz, out_len, t in members]
    starts, batch = G.layout(caps)
    a, b = M.Scanner(env.db), M.Scanner(env.db)
    try:
        a.set_tally(True); b.set_tally(True)
        r = a.scan_gz([gz for gz, _, _ in members], want_text=mode != FETCH_COUNTS, out_lens=[o for _, o, _ in members], fetch_mode=mode)
        b.set_segments(starts)
        want = b.scan(batch)
        assert r.n_hits == want.n_hits and table(r) == table(want) and r.n_hits > 200
        assert r.on_device == (mode == FETCH_DEVICE)
        assert (r.gz_text() == batch) if mode != FETCH_COUNTS else (r.gz_text() is None and r.gz_text_len() == len(batch))
        if mode & 1:
            assert np.array_equal(records(r), records(want))
        if mode == FETCH_HITS | FETCH_COMPACT:
            assert r.n_ip4_hits > 0
        if mode == FETCH_SORTED:
            assert r.hits() == want.hits() and r.segment_of == want.segment_of
        ta, tb = a.tally(), b.tally()
        assert list(ta) == list(tb) and (ta.distinct, ta.matches) == (tb.distinct, tb.matches) and ta.matches == r.n_hits
        r.close(); want.close()
    finally:
        a.close(); b.close()


def test_bad_tables_leave_the_scanner_usable(env):
    M = env.M
    L = M.lib()
    g = G.good_cases()[2]
    raw = M._ScanResult()
    table1 = (M._GzMember * 1)()
    for offset, length, out_len, n in ((len(g[1]) + 1, 0, 0, 1), (1, len(g[1]), 0, 1), (0, len(g[1]), 0, 0), (0, len(g[1]), 0x7FFFFFFF, 1)):
        table1[0].offset, table1[0].len, table1[0].out_len = offset, length, out_len
        assert L.matchy_scanner_scan_gz(env.sc._h, g[1], len(g[1]), table1, n, 1, False, C.byref(raw)) == -5
        assert M.last_error()
    status, _ = check_pack(env, [(g[1], g[2], g[4])])
    assert status == [0]


def test_multi_scanner_in_submission_order(env):
    """two workers on one device: gz batches come back in submission order with the inflated text as data / len, NULL / the length
    without want_text"""
    M = env.M
    ms = M.MultiScanner(env.db, devices=(0, 0))
    try:
        packs, keep = [], []
        for k in range(5):
            texts = [G.log(2 + (i + k) % 6, seed=100 + 10 * k + i) for i in range(3 + k)]
            files = [G.gz_wrap(G.raw_deflate(t), t) for t in texts]
            if k == 3:
                files[1] = files[1][:-9] + files[1][-8:]   # a byte of the body is gone
                texts[1] = None
            packed = C.create_string_buffer(b"".join(files), sum(map(len, files)))
            keep.append(packed)
            table_, pos = [], 0
            for f in files:
                table_.append((pos, len(f), 0))
                pos += len(f)
            caps = []
            for f, t in zip(files, texts):
                isize = int.from_bytes(f[-4:], "little")
                caps.append((isize, t))
            packs.append((texts, caps))
            ms.submit_gz_ptr(C.addressof(packed), len(packed.raw), table_, want_text=k != 2, tag=k)
            if ms.pending() >= ms.max_pending():
                pytest.fail("five batches fit the in-flight bound of two workers")
        for k, (texts, caps) in enumerate(packs):
            b = ms.next(want_hits=True)
            starts, batch = G.layout(caps)
            assert (b["seq"], b["tag"]) == (k, k)
            assert [s == 0 for s in b["gz_status"]] == [t is not None for t in texts]
            assert b["nbytes"] == len(batch) and b["text"] == (batch if k != 2 else None)
            want_recs, want_table, _ = reference(env, starts, batch, False)
            assert [tuple(s.values()) for s in b["segments"]] == want_table
            assert sorted(h["start"] for h in b["hits"]) == sorted(want_recs[:, 0].tolist()) and b["segment_of"] == want_recs[np.argsort(want_recs[:, 0], kind="stable"), 4].tolist()
        assert ms.next() is None
    finally:
        ms.close()
