"""GPU: pieces of one DEFLATE stream (matchy_scanner_set_gz_pieces, csrc/inflate_pieces.hip). zlib gives the expected statuses and
text; the same call with pieces off and the segmented scan of zlib's text give the expected hits; the CPU driver of the piece rules
(tests/cpp/test_gz_pieces.cpp, built here as a plain program) gives the expected piece table, field for field. The hostile vectors run
here only behind tests/test_gz_pieces_host.py, which drives the same rules under a sanitizer."""
import gzip

import numpy as np
import pytest

import gz_cases as G
import gz_pieces_cases as P
from test_gpu_gz import Env, records, reference, table

pytestmark = pytest.mark.gpu

CASES = P.cases()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.sc.set_gz_pieces(0)
    e.sc.close(); e.ref.close(); e.db.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return P.build_driver(tmp_path_factory.mktemp("gz_pieces_gpu"))


def scan(env, blobs, piece_bytes, out_lens=None, files=False):
    env.sc.set_gz_pieces(piece_bytes)
    env.sc.set_line_context(True)
    r = env.sc.scan_gz_files(blobs, want_text=True) if files else env.sc.scan_gz(blobs, want_text=True, out_lens=out_lens)
    out = dict(status=r.gz_status(), text=r.gz_text(), recs=records(r), table=table(r), lines=r.lines, bytes=r.bytes, pieces=r.gz_pieces(),
               file_status=r.gz_file_status() if files else None)
    r.close()
    return out


def same_scan(a, b):
    assert a["status"] == b["status"] and a["text"] == b["text"] and a["table"] == b["table"] and (a["lines"], a["bytes"]) == (b["lines"], b["bytes"])
    assert np.array_equal(a["recs"], b["recs"])


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_vectors(env, driver, tmp_path, k):
    """every vector with pieces on: zlib's status and text, the hits of the call with pieces off and of the oracle on zlib's text, and the
    CPU driver's piece table"""
    name, gz, piece_bytes, status, text = CASES[k]
    on, off = scan(env, [gz], piece_bytes), scan(env, [gz], 0)
    assert [G.STATUS[s] for s in on["status"]] == [status]
    cap = G.plan_status_cap(gz, 0)[1]
    starts, batch = G.layout([(cap, text)])
    assert on["text"] == batch
    same_scan(on, off)
    want_recs, want_table, _ = reference(env, starts, batch, True)
    assert np.array_equal(on["recs"], want_recs) and on["table"] == want_table
    assert off["pieces"] == ([], None)
    pieces, first = on["pieces"]
    (_, _, want), = P.run_driver(driver, tmp_path, [(gz, 0)], piece_bytes)
    assert first == [0, len(want)] and pieces == want
    print(f"{name}: {len(pieces)} pieces, {sum(1 for p in pieces if p[5] & P.LIVE)} live, {len(on['recs'])} hits")


def test_mixed_pack(env, driver, tmp_path):
    """a small member that is not split, two split members side by side, a failed member (the dictionary), and a split member behind
    them: scratch regions and out_pos stay disjoint, segments, lines and bytes are those of the run with pieces off"""
    by = {c[0]: c for c in CASES}
    small = gzip.compress(G.log(20, seed=3))
    names = ["v4_seam", "v4_short_pieces", "v6_dict_later", "v4_run"]
    blobs = [small] + [by[n][1] for n in names]
    texts = [G.log(20, seed=3)] + [by[n][4] for n in names]
    on, off = scan(env, blobs, 512), scan(env, blobs, 0)
    assert [G.STATUS[s] for s in on["status"]] == ["OK", "OK", "OK", "BAD_DISTANCE", "OK"]
    starts, batch = G.layout([(G.plan_status_cap(b, 0)[1], t) for b, t in zip(blobs, texts)])
    assert on["text"] == batch and starts[1] != 0
    same_scan(on, off)
    pieces, first = on["pieces"]
    assert first[0] == first[1] == 0 and first[-1] == len(pieces)
    for i, b in enumerate(blobs[1:], 1):
        (_, _, want), = P.run_driver(driver, tmp_path, [(b, 0)], 512, tag=str(i))
        got = pieces[first[i]:first[i + 1]]
        assert [p[:2] + p[3:] for p in got] == [p[:2] + p[3:] for p in want] and all(p[2] == i for p in got), i
    assert all(p[5] & P.HANDED for p in pieces[first[3]:first[4]]) and not any(p[5] & P.HANDED for p in pieces[first[4]:])


def test_files_with_two_split_members(env):
    """matchy_scanner_scan_gz_files: both members of one file are split; the file is one segment"""
    by = {c[0]: c for c in CASES}
    blob, text = by["v4_seam"][1] + by["v4_short_pieces"][1], by["v4_seam"][4] + by["v4_short_pieces"][4]
    on, off = scan(env, [blob], 512, files=True), scan(env, [blob], 0, files=True)
    assert on["status"] == [0, 0] and on["file_status"] == [0] and on["text"] == text + b"\n"
    same_scan(on, off)
    pieces, first = on["pieces"]
    assert len(first) == 3 and first[1] - first[0] >= 10 and first[2] - first[1] >= 10
    assert sum(1 for p in pieces if p[5] & P.LIVE) >= 16 and not any(p[5] & P.HANDED for p in pieces)


def test_window_with_a_split_member(env):
    """matchy_scanner_scan_gz_window goes through the same inflate stage: the setting applies to it"""
    by = {c[0]: c for c in CASES}
    blob, text = by["v4_short_pieces"][1], by["v4_short_pieces"][4]
    out = []
    for pb in (512, 0):
        env.sc.set_gz_pieces(pb)
        r = env.sc.scan_gz_window(blob, carry=b"partial line ", last=True, want_text=True)
        out.append((r.gz_status(), r.gz_text(), r.gz_window(), r.n_hits, r.gz_pieces()))
        r.close()
    assert out[0][:4] == out[1][:4] and out[0][0] == [0] and out[0][1] == b"partial line " + text + b"\n"
    assert sum(1 for p in out[0][4][0] if p[5] & P.LIVE) >= 8 and out[1][4] == ([], None)


def test_mutant_sample(env):
    """v7, a fixed sample of 256 in one pack: rejected by zlib -> the status of the same call with pieces off, not OK; accepted -> OK and
    zlib's bytes. Every odd member is the pristine stream, so a wave that writes outside its member damages bytes that are compared."""
    gz, text = P.mutant_source()
    muts = [P.mutant_at(gz, i) for i in P.mutant_sample()]
    assert len(muts) == 256
    blobs, want = [], []
    for m in muts:
        blobs += [m, gz]
        want += [P.verdict(m), (True, text)]
    lens = [len(text)] * len(blobs)
    on, off = scan(env, blobs, P.MUTANT_PIECE_BYTES, out_lens=lens), scan(env, blobs, 0, out_lens=lens)
    same_scan(on, off)
    starts, _ = G.layout([(len(text), text)] * len(blobs))
    for i, (ok, t) in enumerate(want):
        assert (on["status"][i] == 0) == ok, i
        got = on["text"][starts[i]:starts[i] + len(text) + 1]
        assert got == ((t if ok else b"\n" * len(text)) + b"\n"), i
    pieces, first = on["pieces"]
    assert first[-1] == len(pieces) and sum(1 for i in range(len(blobs)) if first[i + 1] > first[i]) >= 500


def test_setter_errors_leave_the_scanner_usable(env):
    M = env.M
    env.sc.set_gz_pieces(1024)
    for bad in (3, 2 << 20, 256, 768):
        with pytest.raises(ValueError):
            env.sc.set_gz_pieces(bad)
        assert M.lib().matchy_scanner_set_gz_pieces(env.sc._h, bad) != 0 and "power of two" in M.last_error()
        assert env.sc.gz_pieces() == 1024
    name, gz, _, _, text = CASES[8]
    out = scan(env, [gz], 1024)
    assert out["status"] == [0] and out["text"] == text + b"\n"
    for good in (512, 1 << 20, 0):
        env.sc.set_gz_pieces(good)
        assert env.sc.gz_pieces() == good


def test_off_launches_no_piece_kernel(env):
    """with the setting at 0 the timing getter reads all zeros and the piece table is empty; with it on, the kernels have run"""
    gz = CASES[8][1]
    keep, env.sc = env.sc, env.M.Scanner(env.db, profile=True)
    try:
        scan(env, [gz], 512)
        t = env.sc.gz_pieces_timing_ms()
        assert all(t[k] > 0 for k in ("find", "count", "chain", "symbols", "resolve")) and t["handover"] >= 0
        out = scan(env, [gz], 0)
        assert out["pieces"] == ([], None) and all(v == 0 for v in env.sc.gz_pieces_timing_ms().values())
        out = scan(env, [gzip.compress(G.log(20, seed=3))], 512)   # pieces on, nothing large enough to split
        assert out["pieces"] == ([], [0, 0]) and all(v == 0 for v in env.sc.gz_pieces_timing_ms().values())
    finally:
        env.sc.close()
        env.sc = keep
