"""CPU: the decoding rules of the unescape front pass (matchy_amd/csrc/unescape_core.h), driven by tests/cpp/test_unescape.cpp, compiled
with g++ under -fsanitize=address,undefined as a stand-alone program. The tile-state, count and write functions run tile by tile, the
way the kernels partition the work, over every case of tests/unescape_cases.py and over inputs of several tiles; the pure-Python
reference of that file is the oracle, and urllib and json check the oracle. This run comes in front of any GPU run of the same cases.
No GPU."""
import json
import re
import struct
import subprocess
import urllib.parse

import pytest

import unescape_cases as U
from test_inflate_core_host import build


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("unescape"), "test_unescape")


def test_percent_reference_against_urllib():
    """the oracle equals urllib.parse.unquote_to_bytes, with the LF escapes of the input rewritten to %20, on EVERY generated percent case"""
    n = 0
    for modes, data in U.generated_cases():
        if modes != U.PERCENT:
            continue
        n += 1
        text, escapes, replaced, lf = U.reference(data, U.PERCENT)
        assert text == urllib.parse.unquote_to_bytes(re.sub(rb"%0[aA]", b"%20", data)), data
        assert replaced == 0 and lf == len(re.findall(rb"%0[aA]", data)) and len(text) == len(data) - 2 * escapes
    assert n >= 2000


def json_value(data):
    """the UTF-8 bytes of the JSON string with body `data`, or None where it is no valid body or holds an LF escape or a lone surrogate"""
    try:
        s = json.loads('"' + data.decode("utf-8") + '"')
    except (ValueError, UnicodeDecodeError):
        return None
    if not isinstance(s, str) or "\n" in s or any(0xD800 <= ord(ch) <= 0xDFFF for ch in s):
        return None
    return s.encode("utf-8")


def test_json_reference_against_json_loads():
    """the oracle equals json.loads on every generated JSON case that is a valid string body without LF escapes and lone surrogates; by
    the generator's construction these are at least half of the JSON cases"""
    n = valid = 0
    for modes, data in U.generated_cases():
        if modes != U.JSON:
            continue
        n += 1
        want = json_value(data)
        if want is None:
            continue
        valid += 1
        text, _, replaced, lf = U.reference(data, U.JSON)
        assert text == want and replaced == 0 and lf == 0, data
    print(f"{n} generated JSON cases, {valid} compared with json.loads ({100 * valid / n:.1f} %)")
    assert n >= 2000 and valid >= n / 2
    assert len(U.generated_cases()) >= 4000


def test_named_cases_by_hand():
    """the sequences the rules name, against bytes written out by hand"""
    for name, modes, data, text in U.named_cases():
        assert U.reference(data, modes)[0] == text, name
    by_name = {name: (modes, data) for name, modes, data, _ in U.named_cases()}
    assert U.reference(*reversed(by_name["high high low"]))[1:] == (3, 1, 0)
    assert U.reference(*reversed(by_name["low low"]))[1:] == (2, 2, 0)
    assert U.reference(*reversed(by_name["\\n%0A in both"]))[1:] == (2, 0, 2)
    assert U.reference(*reversed(by_name["\\u002541 in both"]))[1:] == (2, 0, 0)   # one escape in each run


def test_properties_on_every_case():
    """the LF bytes of the input are those of the text, the text is never longer than the input, and decoding is line-local: the text
    of the whole equals the texts of its lines (cut behind every LF), joined"""
    for name, modes, data in U.all_inputs() + U.long_inputs():
        text, escapes, replaced, lf = U.reference(data, modes)
        assert text.count(b"\n") == data.count(b"\n") and len(text) <= len(data), name
        lines = data.split(b"\n")
        pieces = [line + b"\n" for line in lines[:-1]] + [lines[-1]]
        parts = [U.reference(p, modes) for p in pieces]
        assert b"".join(p[0] for p in parts) == text, name
        assert tuple(sum(p[k] for p in parts) for k in (1, 2, 3)) == (escapes, replaced, lf), name


def test_tile_passes_match_the_reference(driver, tmp_path):
    """tile_state_code, tile_count and tile_write over every case and over inputs of several tiles, tile by tile: the bytes and the
    counters are the reference's"""
    inputs = U.all_inputs() + U.long_inputs()
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    U.write_case_file(src, inputs)
    r = subprocess.run([str(driver), "cases", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and "unescape cases ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    raw, pos = dst.read_bytes(), 0
    for name, modes, data in inputs:
        n, escapes, replaced, lf = struct.unpack_from("<IIII", raw, pos)
        pos += 16
        assert (raw[pos:pos + n], escapes, replaced, lf) == U.reference(data, modes), name
        pos += n
    assert pos == len(raw)
