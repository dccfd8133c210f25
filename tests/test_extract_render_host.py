"""CPU: the rules of `matchy extract`'s output that host and kernels share (matchy_amd/csrc/extract_render_core.h: order key, type rank,
record length, record writer), compiled with g++ under -fsanitize=address,undefined as a stand-alone program
(tests/cpp/test_extract_render_core.cpp) and held against the Python model of tests/extract_render_cases.py; and the C ABI surface of
the feature (header, export list, library). No GPU."""
import random
import re
import subprocess
from pathlib import Path

import pytest

from extract_render_cases import FORMATS, LINE_BITS, RANK, RANK_BITS, START_BITS, TYPE_NAMES, key, record

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

MATCHY_ERROR_INVALID_PARAM = -5
NEW_FUNCTIONS = ["matchy_amd_extractor_extract_rendered", "matchy_amd_extractor_get_render_timing", "matchy_amd_extractor_render_allocations"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("extract_render_core") / "test_extract_render_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", str(CSRC),
                    str(ROOT / "tests" / "cpp" / "test_extract_render_core.cpp"), "-o", str(exe)], check=True)
    return exe


def run(driver, *args):
    r = subprocess.run([str(driver), *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "extract_render_core ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout.splitlines()[:-1]


def texts():
    """a quote and a backslash at the first, the last and every inner position of a text; both next to each other; the empty text"""
    base = b"ab.c-d7"
    out = [b"", base, b'"', b"\\", b'"\\', b'\\"', b'""', b"\\\\", b'a"\\b', bytes(range(1, 48))]
    for ch in (b'"', b"\\"):
        for at in range(len(base)):
            out.append(base[:at] + ch + base[at + 1:])   # in place of a byte
            out.append(base[:at] + ch + base[at:])       # in front of it
        out.append(base + ch)
    return out


def test_every_type_format_and_escape_position(driver, tmp_path):
    cases = [(f, t, x) for f in FORMATS for t in range(12) for x in texts()]
    path = tmp_path / "render.txt"
    path.write_text("".join("%d %d %s\n" % (FORMATS[f], t, x.hex() or "-") for f, t, x in cases))
    rows = run(driver, "render", path)
    assert len(rows) == len(cases) == 3 * 12 * len(texts())
    for (f, t, x), row in zip(cases, rows):
        n, hx = (row.split() + [""])[:2]
        want = record(f, t, x)
        assert (int(n), bytes.fromhex(hx)) == (len(want), want), (f, t, x)


def test_random_texts(driver, tmp_path):
    rng = random.Random(20260101)
    alphabet = b'"\\ab,\n\r\t{}:\x00\x7f\xc3\xa9'
    cases = [(rng.choice(list(FORMATS)), rng.randrange(12), bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 40)))) for _ in range(3000)]
    path = tmp_path / "random.txt"
    path.write_text("".join("%d %d %s\n" % (FORMATS[f], t, x.hex() or "-") for f, t, x in cases))
    rows = run(driver, "render", path)
    assert len(rows) == len(cases)
    for (f, t, x), row in zip(cases, rows):
        hx = (row.split() + [""])[1]
        assert bytes.fromhex(hx) == record(f, t, x), (f, t, x)


def test_names_ranks_and_field_widths(driver):
    rows = run(driver, "types")
    assert rows[-1] == "bits %d %d %d max_len %d" % (LINE_BITS, RANK_BITS, START_BITS, 1 << START_BITS)
    for t in range(12):
        assert rows[t].split() == [str(t), str(RANK[t]), TYPE_NAMES[t].lower()]
    assert rows[12].split() == ["12", "4", "unknown"]
    assert sorted(set(RANK.values())) == list(range(8))


def test_key_pack_and_unpack_at_the_field_limits(driver, tmp_path):
    limits = [(line, rank, start) for line in (0, 1, (1 << LINE_BITS) - 1) for rank in range(1 << RANK_BITS) for start in (0, 1, (1 << START_BITS) - 1)]
    path = tmp_path / "limits.txt"
    path.write_text("".join("%d %d %d\n" % t for t in limits))
    rows = run(driver, "keys", path)
    assert len(rows) == len(limits)
    for t, row in zip(limits, rows):
        assert tuple(map(int, row.split())) == (key(*t), *t)
    assert key((1 << LINE_BITS) - 1, 7, (1 << START_BITS) - 1) == (1 << 64) - 1


def test_key_order_is_tuple_order(driver, tmp_path):
    rng = random.Random(7)
    small = [(rng.randrange(4), rng.randrange(8), rng.randrange(6)) for _ in range(2000)]   # many ties in every field
    wide = [(rng.randrange(1 << LINE_BITS), rng.randrange(8), rng.randrange(1 << START_BITS)) for _ in range(2000)]
    triples = small + wide
    path = tmp_path / "order.txt"
    path.write_text("".join("%d %d %d\n" % t for t in triples))
    keys = [int(row.split()[0]) for row in run(driver, "keys", path)]
    assert len(keys) == len(triples)
    assert sorted(range(len(triples)), key=lambda i: (keys[i], i)) == sorted(range(len(triples)), key=lambda i: (triples[i], i))
    for i in range(0, len(triples) - 1):
        a, b = triples[i], triples[i + 1]
        assert (keys[i] < keys[i + 1], keys[i] == keys[i + 1]) == (a < b, a == b)


def test_header_export_list_and_library_carry_the_entry():
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"int32_t\s+matchy_amd_extractor_extract_rendered\s*\(\s*const matchy_extractor_t\s*\*\s*\w+,\s*const uint8_t\s*\*\s*\w+,\s*uintptr_t\s+\w+,\s*uint32_t\s+\w+\s*(?:/\*[^*]*\*/)?\s*,"
                     r"\s*matchy_amd_extract_text_t\s*\*\s*\w+\s*\)", header)
    assert re.search(r"typedef struct matchy_amd_extract_text_t \{[^}]*by_type\[12\][^}]*status[^}]*\}", header)
    # invalid parameters need no device: a null handle, a null out
    import ctypes as C
    out = M._ExtractText()
    assert L.matchy_amd_extractor_extract_rendered(None, b"x", 1, 0, C.byref(out)) == MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_amd_extractor_render_allocations(None) == 0
    assert hasattr(M.Extractor, "extract_rendered")


def test_command_line_names_the_flag():
    import matchy_amd.build as B
    src = "".join((CSRC / name).read_text() for name in B.CLI_SOURCES)
    assert "--render-on-gpu" in src and "matchy_amd_extractor_extract_rendered" in src
    assert "extract_render.hip" in B.SOURCES
