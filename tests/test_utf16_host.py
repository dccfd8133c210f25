"""CPU: the transcoding rules of the UTF-16 front pass (matchy_amd/csrc/utf16_core.h) and the 16-bit cut rule and reader of
csrc/batch_reader.h, driven by tests/cpp/test_utf16.cpp, compiled with g++ under -fsanitize=address,undefined as a stand-alone program.
The count and write functions run tile by tile, the way the kernels partition the work, over every case of tests/utf16_cases.py; the
pure-Python reference of that file is the oracle, and the interpreter's own codec checks the oracle. This run comes in front of any GPU
run of the same cases. No GPU."""
import random
import struct
import subprocess

import pytest

import utf16_cases as U
from test_inflate_core_host import build


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("utf16"), "test_utf16")


def test_reference_against_the_codec():
    """the oracle agrees with bytes.decode(..., 'replace') on every case except odd-length inputs whose last whole unit is a high
    surrogate (CPython writes one U+FFFD for those two errors, the rules write two): the only exclusion, at most 5 % of the generated cases"""
    excluded = generated = 0
    for name, order, data in U.all_inputs():
        is_generated = name.startswith("generated")
        generated += is_generated
        text, units, replaced = U.reference(data, order)
        assert units == len(data) // 2 and text.count(U.FFFD) >= replaced
        if U.codec_differs_by_rule(data, order):
            excluded += is_generated
            assert text == U.codec(data[:-1], order) + U.FFFD, name   # the codec on the whole units, then the odd byte's own U+FFFD
            continue
        assert text == U.codec(data, order), name
    share = excluded / generated
    print(f"{generated} generated cases, {excluded} excluded from the codec comparison ({100 * share:.1f} %)")
    assert generated >= 4000 and 0 < share <= 0.05


def test_named_cases_by_hand():
    """the sequences the rules name, against bytes written out by hand"""
    H, L = 0xD800, 0xDC00
    for order in (U.LE, U.BE):
        def ref(units, odd=None):
            return U.reference(U.encode_units(units, order, odd), order)
        assert ref([]) == (b"", 0, 0)
        assert ref([], 0x41) == (U.FFFD, 0, 1)
        assert ref([H, L]) == (b"\xf0\x90\x80\x80", 2, 0)
        assert ref([0xDBFF, 0xDFFF]) == (b"\xf4\x8f\xbf\xbf", 2, 0)
        assert ref([H, H, L]) == (U.FFFD + b"\xf0\x90\x80\x80", 3, 1)
        assert ref([L, L]) == (U.FFFD * 2, 2, 2)
        assert ref([0x41, H]) == (b"A" + U.FFFD, 2, 1)
        assert ref([L, 0x41]) == (U.FFFD + b"A", 2, 1)
        assert ref([0x41, H], 0xDC) == (b"A" + U.FFFD * 2, 2, 2)
        assert ref([0xFEFF]) == (b"\xef\xbb\xbf", 1, 0) and ref([0xFFFE]) == (b"\xef\xbf\xbe", 1, 0)
        assert ref([0x7F, 0x80, 0x7FF, 0x800, 0xFFFF]) == (b"\x7f\xc2\x80\xdf\xbf\xe0\xa0\x80\xef\xbf\xbf", 5, 0)


def long_inputs():
    """inputs of several tiles: pool units at random, so that pairs and lone surrogates fall on tile boundaries; pairs only; odd lengths"""
    rng = random.Random(99)
    out = []
    for k, n in enumerate([511, 512, 513, 1024, 1500, 3000]):
        for order in (U.LE, U.BE):
            units = [rng.choice(U.POOL) for _ in range(n)]
            out.append((f"long {k}", order, U.encode_units(units, order, 0xD8 if k % 2 else None)))
    for order in (U.LE, U.BE):
        out.append(("pairs", order, U.encode_units([0xD83D, 0xDE00] * 700, order)))
        out.append(("pairs shifted", order, U.encode_units([0x41] + [0xD83D, 0xDE00] * 700, order)))   # every tile boundary splits a pair
        out.append(("ffff", order, U.encode_units([0xFFFF] * 1100, order)))
        # the most a tile can give: three bytes of every unit but the last, and all four of a pair whose low surrogate opens the next tile
        out.append(("full tile + pair across", order, U.encode_units([0x20AC] * 511 + [0xD83D, 0xDE00] + [0x20AC] * 511 + [0xDBFF, 0xDFFF] + [0x20AC] * 30, order)))
    return out


def test_tile_passes_match_the_reference(driver, tmp_path):
    """tile_count and tile_write over every case, tile by tile: the bytes and the U+FFFD count are the reference's"""
    inputs = U.all_inputs() + long_inputs()
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    U.write_case_file(src, inputs)
    r = subprocess.run([str(driver), "cases", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and "utf16 cases ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    raw, pos = dst.read_bytes(), 0
    for name, order, data in inputs:
        n, replaced = struct.unpack_from("<II", raw, pos)
        pos += 8
        text, _, want_replaced = U.reference(data, order)
        assert (raw[pos:pos + n], replaced) == (text, want_replaced), name
        pos += n
    assert pos == len(raw)


def test_cut_rule_and_reader(driver):
    """newline_cut16: cuts only behind 000A at even offsets, U+0A41 and xx00 0Ayy are no cuts, a line longer than the window; the reader
    with reads of one byte at a time equals cutting the whole buffer"""
    r = subprocess.run([str(driver), "cuts"], capture_output=True, text=True)
    assert r.returncode == 0 and "utf16 cuts ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
