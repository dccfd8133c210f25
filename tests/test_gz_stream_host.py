"""CPU: the rules of stream windows (matchy_amd/csrc/inflate_core.h "windows of one stream") and the walker of csrc/gz_stream.h, driven
sequentially through all passes by tests/cpp/test_gz_stream.cpp, compiled with g++ under -fsanitize=address,undefined as a stand-alone
program and fed the vectors of tests/gz_pieces_cases.py as chains of windows. This run comes in front of any GPU run of the same vectors:
a load outside a window's compressed bytes, or a store outside a piece's own range of the symbols or outside the text capacity, stops
the sanitized program. zlib in the interpreter is the reference. No GPU."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import gz_cases as G
import gz_pieces_cases as P
import gz_stream_cases as S
from test_inflate_core_host import ROOT, build

INVALID = -5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("gz_stream"), "test_gz_stream")


@pytest.fixture(scope="module")
def chains(driver, tmp_path_factory):
    """every chain of S.CHAINS through the driver, once: name -> [Window]"""
    tmp = tmp_path_factory.mktemp("gz_stream_run")
    return {name: S.run_chains(driver, tmp, [S.vector(name)[0]], chain, tag=name)[0] for name, chain in S.CHAINS.items()}


def test_walker_rules(driver):
    """gz_stream.h on synthetic numbers: first window, next start, the ratio and its clamps, the file's end, a device that claims no
    progress; the ISIZE comparison just below and just above 2^32 and the trailer's precedence"""
    r = subprocess.run([str(driver), "walker"], capture_output=True, text=True)
    assert r.returncode == 0 and "gz_stream walker ok" in r.stdout, r.stdout + r.stderr[-4000:]


def test_chains_are_zlibs(chains):
    """texts, consumed bits, states and `ended` of every OK vector (S.check_chain)"""
    for name, chain in chains.items():
        gz, text = S.vector(name)
        assert P.verdict(gz) == (True, text)
        S.check_chain(chain, gz, text)
        print(f"{name}: {len(gz)} bytes in {len(chain)} windows, {sum(w.bit != 0 for w in chain)} not byte aligned, {sum(w.cut_by_cap for w in chain)} cut by the capacity, "
              f"{sum(w.history_markers for w in chain)} markers of piece 0 from the history")


def test_windows_that_would_hide_a_failure(chains):
    """without these the chains could pass with one window that holds everything, or with windows that never start inside a byte"""
    z = chains["v2_zblock"]
    assert len(z) >= 10 and any(w.cut_by_cap for w in z) and sum(w.bit != 0 for w in z) >= 9
    assert all(not w.flags & S.FILE_END for w in z if w.cut_by_cap)
    assert len(chains["v1_l6"]) >= 3
    seam = chains["v4_seam"]
    assert any(w.history_markers for w in seam)
    # the hand-made match of distance 32768 lies at len(a) (gz_pieces_cases.seam_case): the window that holds it starts behind its
    # source, with a history of the full 32 KiB in front of it
    a = len(G.log(600, seed=21))
    done = 0
    for w in seam:
        if done <= a < done + w.text_len:
            assert done >= 32768 and a - 32768 < done and w.history_markers, (a, done)
            break
        done += w.text_len
    else:
        raise AssertionError("no window holds the seam")
    for name, chain in chains.items():
        for w in chain:
            live = [p for p in w.pieces if p[5] & P.LIVE]
            assert live and live[0][0] == w.bit, name
            for x, y in zip(live, live[1:]):
                assert y[0] == x[1] and y[4] == x[4] + x[3], name


def test_no_progress_and_failures(driver, tmp_path):
    fixed, _ = S.vector("v3_fixed")
    (c,) = S.run_chains(driver, tmp_path, [fixed], (8 << 10, 1024, 1 << 20), tag="fixed")
    assert [(w.status, w.gz_status, w.text_len, w.consumed_bits) for w in c] == [("NO_PROGRESS", "OK", 0, 0)]
    # the whole of it in one window is piece 0's alone, and the stream's end
    (c,) = S.run_chains(driver, tmp_path, [fixed], (1 << 20, 1024, 1 << 20), tag="fixed1")
    assert len(c) == 1 and c[0].status == "OK" and c[0].ended and c[0].text == S.vector("v3_fixed")[1]
    # a capacity below the first block's text (20 000 bytes)
    z, _ = S.vector("v2_zblock")
    (c,) = S.run_chains(driver, tmp_path, [z], (16 << 10, 1024, 19999), tag="cap")
    assert [(w.status, w.gz_status) for w in c] == [("NO_PROGRESS", "OK")]
    (c,) = S.run_chains(driver, tmp_path, [z], (16 << 10, 1024, 20000), tag="cap1")
    assert c[0].status == "OK" and c[0].text_len == 20000
    # the preset dictionary: piece 0 of the first window, whose history is empty
    d, _ = S.vector("v6_dict_piece0")
    (c,) = S.run_chains(driver, tmp_path, [d], (4 << 10, 512, 64 << 10), tag="dict")
    assert [(w.status, w.gz_status) for w in c] == [("FAILED", "BAD_DISTANCE")]
    # ... and behind 9000 bytes that need none: a marker points in front of the history, in whichever window meets it first
    d, _ = S.vector("v6_dict_later")
    (c,) = S.run_chains(driver, tmp_path, [d], (4 << 10, 512, 64 << 10), tag="dict2")
    assert all(w.status == "OK" for w in c[:-1]) and (c[-1].status, c[-1].gz_status) == ("FAILED", "BAD_DISTANCE")
    assert sum(w.text_len for w in c) < 9000 + 32768
    # a header that does not parse
    (c,) = S.run_chains(driver, tmp_path, [b"\x1f\x8c" + z[2:]], (16 << 10, 1024, 48 << 10), tag="hdr")
    assert [(w.status, w.gz_status) for w in c] == [("FAILED", "BAD_HEADER")]


@pytest.mark.parametrize("name", ["v2_zblock", "v4_seam"])
def test_trailer_mutants_fail_in_the_last_window(driver, tmp_path, chains, name):
    good = chains[name]
    for what, gz, status in S.trailer_mutants(name):
        (c,) = S.run_chains(driver, tmp_path, [gz], S.CHAINS[name], tag=what)
        assert len(c) == len(good) and all(w.status == "OK" and not w.ended for w in c[:-1]), what
        assert (c[-1].status, c[-1].gz_status, c[-1].text_len) == ("FAILED", status, 0), what
        assert [w.text for w in c[:-1]] == [w.text for w in good[:-1]]
        assert not P.verdict(gz)[0]


def test_mutants(driver, tmp_path):
    """every single-bit flip and every proper prefix of P.mutant_source(): the chain is zlib's text, or it stops at a window that is not
    OK; what the windows in front of it gave is the true text at least up to the block the flip lies in (a window may hold a flipped
    literal: its CRC is the last window's to refuse). Nothing stops the sanitized program."""
    gz, text = P.mutant_source()
    (good,) = S.run_chains(driver, tmp_path, [gz], S.MUTANT_CHAIN, tag="pristine")
    S.check_chain(good, gz, text)
    assert len(good) >= 3
    bounds = S.boundaries(good)
    muts = P.mutants()
    h = G.header_len(gz)
    flips = (len(gz) - h) * 8
    workers = max(1, min(8, os.cpu_count() or 1))
    chunks = [list(range(k, len(muts), workers)) for k in range(workers)]
    with ThreadPoolExecutor(workers) as pool:
        done = list(pool.map(lambda k: S.run_verdicts(driver, tmp_path, [muts[i] for i in chunks[k]], S.MUTANT_CHAIN, text, tag="m%d" % k), range(workers)))
    whole = stopped = 0
    for k, got in enumerate(done):
        for i, (st, gst, nw, ended, accepted, common) in zip(chunks[k], got):
            ok, ztext = P.verdict(muts[i])
            if ended:
                assert ok and st == "OK" and accepted == common == len(ztext) and ztext == text, i
                whole += 1
                continue
            assert st != "OK" and nw >= 1, i
            stopped += 1
            at = h * 8 + i if i < flips else (h + i - flips) * 8      # the first bit of the file that is not the pristine file's
            sure = max(t for b, t in bounds if b <= at)                # text in front of the block that bit lies in
            assert common >= min(accepted, sure), (i, st, gst, accepted, common, sure)
            assert ok is False or st == "NO_PROGRESS", i               # zlib accepts it: only a refusal to go on is allowed
    print(f"{len(muts)} mutants: {whole} chains reached the stream's end, {stopped} stopped")
    assert whole + stopped == len(muts) and stopped * 10 >= len(muts) * 9


def test_python_walker_follows_gz_stream_h(chains):
    """matchy_amd.GzStreamWalker, fed what the CPU driver's windows reported, asks for the windows the C++ walker asked for"""
    import matchy_amd as M
    for name, chain in chains.items():
        gz, _ = S.vector(name)
        walk = M.GzStreamWalker(len(gz), *S.CHAINS[name])
        for w in chain:
            assert not walk.over and walk.next() == (w.offset, w.len, w.bit, w.flags), name
            assert walk.accept(walk.next(), w.consumed_bits, w.text_len, bool(w.ended))
        assert walk.over and walk.ended and walk.windows == len(chain) and walk.text_bytes == sum(w.text_len for w in chain)
    walk = M.GzStreamWalker(1 << 30, 1 << 20, 512, 50000, first_bytes=4096)
    assert walk.next() == (0, 4096, 0, M.STREAM_FIRST)
    assert walk.accept(walk.next(), 8000, 100000, False) and walk.want == 2048       # the numbers of the driver's walker test
    walk.refuse()
    assert walk.over and not walk.ended


def test_interface_and_refusals_in_front_of_the_scanner():
    """the header, the library and the Python mirror name the same calls and values; every parameter error is refused before the scanner
    handle is followed"""
    import matchy_amd as M
    import matchy_amd.build as B
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in ("matchy_scanner_scan_gz_stream", "matchy_scan_result_gz_stream", "matchy_multi_scanner_submit_gz_stream"):
        assert re.search(r"int32_t\s+%s\s*\(" % name, header) and name in M.EXPORTED_SYMBOLS and getattr(L, name) is not None, name
    assert "matchy_scanner_get_gz_stream_timing" in M.EXPORTED_SYMBOLS and L.matchy_scanner_get_gz_stream_timing is not None
    for name, value in (("FIRST", M.STREAM_FIRST), ("FILE_END", M.STREAM_FILE_END), ("OK", M.STREAM_OK), ("NO_LINE_END", M.STREAM_NO_LINE_END),
                        ("NO_PROGRESS", M.STREAM_NO_PROGRESS), ("FAILED", M.STREAM_FAILED)):
        assert int(re.search(r"#define MATCHY_STREAM_%s (\d+)u?\b" % name, header).group(1)) == value, name
    assert [M.STREAM_OK, M.STREAM_NO_LINE_END, M.STREAM_NO_PROGRESS, M.STREAM_FAILED] == [S.STATUS.index(x) for x in ("OK", "NO_LINE_END", "NO_PROGRESS", "FAILED")]
    assert int(re.search(r"#define MATCHY_STREAM_PASSES (\d+)", header).group(1)) == len(M.GZ_STREAM_PASSES)
    assert C.sizeof(M.GzStreamState) == 24 + 32768 and M.GzStreamState.history.offset == 20 and M.GzStreamState.bit.offset == 12
    assert C.sizeof(M._GzStreamWindow) == 32 and M._GzStreamWindow.carry_len.offset == 16 and M._GzStreamWindow.flags.offset == 28
    for cls, attrs in ((M.Scanner, ("scan_gz_stream", "gz_stream_timing_ms")), (M.MultiScanner, ("submit_gz_stream_ptr",)), (M.ScanResult, ("gz_stream",))):
        for a in attrs:
            assert hasattr(cls, a), (cls, a)
    hip = (ROOT / "matchy_amd" / "csrc" / "inflate_pieces.hip").read_text() + (ROOT / "matchy_amd" / "csrc" / "inflate.hip").read_text()
    for k in ("find", "count", "chain", "symbols", "windows", "resolve", "verdict", "tail"):
        assert re.search(r"__global__[^;{]*\bk_gz_stream_%s\b" % k, hip), k
    assert "hip/" not in (ROOT / "matchy_amd" / "csrc" / "gz_stream.h").read_text()
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in B.CLI_SOURCES)
    assert "--gz-stream-windows" in src and "matchy_multi_scanner_submit_gz_stream" in src and '#include "gz_stream.h"' in src
    raw = M._ScanResult()
    fake = C.c_void_p(8)   # a handle that is never followed
    state = M.GzStreamState(100, 0, 3, 50)

    def window(state=None, carry_len=0, carry_cap=64, text_cap=4096, flags=M.STREAM_FIRST):
        return M._GzStreamWindow(C.pointer(state) if state is not None else None, None, carry_len, carry_cap, text_cap, flags)
    w = window()
    assert L.matchy_scanner_scan_gz_stream(None, b"x", 1, C.byref(w), 1, False, C.byref(raw)) == INVALID and "gz_stream" in M.last_error()
    assert L.matchy_scanner_scan_gz_stream(fake, b"x", 1, C.byref(w), 1, False, None) == INVALID
    assert L.matchy_scanner_scan_gz_stream(fake, b"x", 0, C.byref(w), 1, False, C.byref(raw)) == INVALID and "packed_len" in M.last_error()
    assert L.matchy_scanner_scan_gz_stream(fake, b"x", 1, None, 1, False, C.byref(raw)) == INVALID and "window" in M.last_error()
    for bad, word in ((window(carry_len=65), "carry_cap"), (window(carry_len=3), "NULL"), (window(flags=4), "flag"), (window(flags=0), "state"),
                      (window(state=M.GzStreamState(100, 0, 8, 50), flags=0), "bit"), (window(state=M.GzStreamState(1 << 20, 0, 0, 32769), flags=0), "history_len"),
                      (window(state=M.GzStreamState(49, 0, 0, 50), flags=M.STREAM_FILE_END), "history_len"), (window(text_cap=0), "text_cap"),
                      (window(text_cap=(1 << 31) - 1), "2^31"), (window(carry_cap=1 << 31), "2^31")):
        assert L.matchy_scanner_scan_gz_stream(fake, b"x", 1, C.byref(bad), 1, False, C.byref(raw)) == INVALID and word in M.last_error(), word
        assert L.matchy_multi_scanner_submit_gz_stream(fake, b"x", 1, C.byref(bad), False, None) == INVALID and word in M.last_error(), word
    assert L.matchy_multi_scanner_submit_gz_stream(None, b"x", 1, C.byref(window(state=state, flags=0)), False, None) == INVALID and "gz_stream" in M.last_error()
    assert L.matchy_scan_result_gz_stream(None, None, None, None, None, None, None, None, None) == INVALID
    assert L.matchy_scan_result_gz_stream(C.byref(raw), None, None, None, None, None, None, None, None) == INVALID and "stream window" in M.last_error()
