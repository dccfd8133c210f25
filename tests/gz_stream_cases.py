"""Chains of stream windows (Scanner.scan_gz_stream): what tests/test_gz_stream_host.py and the GPU tests share — the settings of every
chain, the calls that run the CPU driver (tests/cpp/test_gz_stream.cpp) and the reader of its output. The vectors are those of
tests/gz_pieces_cases.py; zlib in the interpreter is the reference.

A chain is (vector name, window_bytes, piece_bytes, text_cap): window_bytes is the walker's first guess and upper bound (gz_stream.h)."""
import struct
import subprocess
import zlib
from collections import namedtuple
from pathlib import Path

import gz_cases as G
import gz_pieces_cases as P

CHAINS = {
    "v2_zblock": (16 << 10, 1024, 48 << 10),        # about three blocks of 20 000 bytes per window: the capacity cuts
    "v1_l6": (64 << 10, 4096, 1 << 20),
    "v4_seam": (4 << 10, 512, 64 << 10),
    "v4_run": (4 << 10, 512, 128 << 10),
    "v4_short_pieces": (4 << 10, 512, 64 << 10),
}
MUTANT_CHAIN = (4 << 10, 1024, 20000)               # blocks of 6000 bytes of text: the capacity cuts here too

Window = namedtuple("Window", "status gz_status consumed_bits text_len ended flags bit offset len base_bit history_markers cut_by_cap "
                              "text_bytes crc state_bit history text pieces")
STATUS = ["OK", "NO_LINE_END", "NO_PROGRESS", "FAILED"]
FIRST, FILE_END = 1, 2

_vectors = {}


def vector(name):
    """(gzip file, text or None)"""
    if not _vectors:
        for n, gz, _, _, text in P.cases():
            _vectors[n] = (gz, text)
    return _vectors[name]


def trailer_mutants(name):
    """[(what, file, expected gz status)]: a flipped byte of the trailer's CRC, one byte of garbage behind the trailer"""
    gz, _ = vector(name)
    m = bytearray(gz)
    m[-6] ^= 0x40
    return [("crc", bytes(m), "CRC_MISMATCH"), ("garbage", gz + b"\x00", "TRAILING_DATA")]


def build_driver(tmp):
    """tests/cpp/test_gz_stream.cpp as a plain program (the sanitized build is test_inflate_core_host.build's)"""
    root = Path(__file__).resolve().parent.parent
    exe = Path(tmp) / "test_gz_stream"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", str(root / "matchy_amd" / "csrc"), str(root / "tests" / "cpp" / "test_gz_stream.cpp"), "-o", str(exe)], check=True)
    return exe


def run_chains(driver, tmp, files, chain, tag=""):
    """files: [gzip file] -> [[Window]]"""
    src, dst = Path(tmp) / ("stream_cases%s.bin" % tag), Path(tmp) / ("stream_out%s.bin" % tag)
    G.write_case_file(src, [(f, 0) for f in files])
    r = subprocess.run([str(driver), str(src), str(dst), *map(str, chain)], capture_output=True, text=True)
    assert r.returncode == 0 and "gz_stream ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    return read_chains(dst.read_bytes(), len(files))


def read_chains(raw, n):
    pos, out = 0, []
    for _ in range(n):
        (nw,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        chain = []
        for _ in range(nw):
            head = struct.unpack_from("<iiQIIIIQQQII", raw, pos)
            pos += struct.calcsize("<iiQIIIIQQQII")
            text_bytes, crc, bit, hl = struct.unpack_from("<QIII", raw, pos)
            pos += 20
            history = raw[pos:pos + hl]
            pos += hl
            text = raw[pos:pos + head[3]]
            pos += head[3]
            (np,) = struct.unpack_from("<I", raw, pos)
            pos += 4
            pieces = [struct.unpack_from("<QQIIII", raw, pos + 32 * k) for k in range(np)]
            pos += 32 * np
            chain.append(Window(STATUS[head[0]], G.STATUS[head[1]], *head[2:], text_bytes, crc, bit, history, text, pieces))
        out.append(chain)
    assert pos == len(raw)
    return out


def run_verdicts(driver, tmp, files, chain, ref, tag=""):
    """files: [gzip file], ref: the true text -> [(status, gz status, n_windows, ended, accepted bytes, common prefix with ref)]"""
    src, dst, rf = Path(tmp) / ("stream_cases%s.bin" % tag), Path(tmp) / ("stream_out%s.bin" % tag), Path(tmp) / ("stream_ref%s.bin" % tag)
    G.write_case_file(src, [(f, 0) for f in files])
    rf.write_bytes(ref)
    r = subprocess.run([str(driver), str(src), str(dst), *map(str, chain), str(rf)], capture_output=True, text=True)
    assert r.returncode == 0 and "gz_stream ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    raw = dst.read_bytes()
    assert len(raw) == 32 * len(files)
    return [(STATUS[s], G.STATUS[g], nw, bool(e), acc, com) for s, g, nw, e, acc, com in struct.iter_unpack("<iiIIQQ", raw)]


def check_chain(chain, gz, text):
    """the assertions every OK chain meets: the windows tile the file bit by bit, the texts are zlib's, the states chain"""
    assert all(w.status == "OK" for w in chain)
    assert b"".join(w.text for w in chain) == text
    assert [w.ended for w in chain] == [0] * (len(chain) - 1) + [1]
    assert chain[0].flags & FIRST and chain[0].offset == 0 and chain[0].bit == 0 and chain[-1].flags & FILE_END
    done = 0
    for k, w in enumerate(chain):
        done += w.text_len
        prefix = text[:done]
        assert w.text_bytes == done and w.crc == zlib.crc32(prefix) and w.history == prefix[-32768:], k
        end = w.offset * 8 + w.consumed_bits          # in bits of the file
        assert w.state_bit == end % 8
        if k + 1 < len(chain):
            assert (chain[k + 1].offset, chain[k + 1].bit) == (end // 8, end % 8), k
            assert not chain[k + 1].flags & FIRST
    assert (chain[-1].offset * 8 + chain[-1].consumed_bits + 7) // 8 + 8 == len(gz)


def boundaries(chain):
    """[(bit of the file, text offset)] of every block start the chain went through, in order"""
    out, done = [], 0
    for w in chain:
        for start, _, _, _, out_pos, flags in w.pieces:
            if flags & P.LIVE:
                out.append((w.base_bit + start, done + out_pos))
        done += w.text_len
    return out
