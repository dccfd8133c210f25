"""CPU: the host side of line context — the C ABI surface (header, export list, library) and the lossy UTF-8 conversion behind
"input_line", compiled alone with g++ under AddressSanitizer + UBSan and compared with bytes.decode("utf-8", "replace"), which
substitutes one U+FFFD per maximal ill-formed subsequence like String::from_utf8_lossy."""
import itertools
import random
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

NEW_FUNCTIONS = ["matchy_scanner_set_line_context", "matchy_scanner_line_context", "matchy_scan_result_lines",
                 "matchy_multi_scanner_set_line_context", "matchy_scan_result_to_ndjson_lines"]


def test_header_export_list_and_library_carry_the_line_context_calls():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    assert "typedef struct matchy_scan_line_t { uint32_t line, line_start, line_end, reserved; } matchy_scan_line_t;" in header
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    # the constants the GPU tests place their edge cases with are the ones the kernels are built with
    lh = (ROOT / "matchy_amd" / "csrc" / "line_index.h").read_text()
    assert int(re.search(r"LINE_TILE = (\d+);", lh).group(1)) == M.LINE_TILE
    assert int(re.search(r"LINE_SCAN_CHUNK = (\d+);", lh).group(1)) == M.LINE_SCAN_CHUNK


def _cases():
    cases = [
        b"", b"a", b"plain ascii line\r", "é".encode(), "€".encode(), "😀".encode(), "aé€😀z".encode(),
        # truncated 2-, 3- and 4-byte sequences, in the middle and at the very end
        b"\xc3", b"a\xc3", b"\xc3a", b"\xe2\x82", b"\xe2\x82a", b"\xe2", b"\xe2a", b"\xf0\x9f\x98", b"\xf0\x9f\x98a", b"\xf0\x9f", b"\xf0\x9fa",
        b"\xf0", b"\xf0a", b"x\xf0\x9f\x98", b"x\xe2\x82",
        # overlongs
        b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",
        # surrogates and beyond U+10FFFF
        b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xed\x9f\xbf", b"\xf4\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf5\x80\x80\x80",
        # lone continuation bytes, 0xFE / 0xFF
        b"\x80", b"\xbf\xbf", b"\xff", b"a\xffb", b"\xfe\xff", b"\xff" * 5,
        # a lead byte followed by another lead byte
        b"\xe2\xe2\x82\xac", b"\xf0\xc3\xa9", b"\xc3\xc3\xa9",
        "GET /a?q=é HTTP/1.1 €\U0001f600".encode() + b"\xff tail",
    ]
    rng = random.Random(20260)
    alphabet = [b"a", b"\x7f", b"\x80", b"\xbf", b"\xc2", b"\xc3", b"\xe0", b"\xa0", b"\xed", b"\x9f", b"\xf0", b"\x90", b"\xf4", b"\x8f", b"\xff", b"\xe2\x82\xac"]
    cases += [b"".join(p) for p in itertools.product(alphabet[:15], repeat=2)]
    cases += [b"".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 12))) for _ in range(2000)]
    return cases


def test_lossy_utf8_matches_python_replace_under_sanitizers(tmp_path):
    exe = tmp_path / "test_utf8_lossy"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "matchy_amd" / "csrc"),
                    str(ROOT / "tests/cpp/test_utf8_lossy.cpp"), "-o", str(exe)], check=True)
    cases = _cases()
    r = subprocess.run([str(exe)], input="".join(c.hex() + "\n" for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert bytes.fromhex(g) == c.decode("utf-8", "replace").encode("utf-8"), c
