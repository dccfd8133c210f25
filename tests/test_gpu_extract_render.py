"""GPU: matchy_amd_extractor_extract_rendered (csrc/extract_render.hip behind Scanner::fetch) against a model that is independent of the
new code: the candidates matchy_extractor_extract_chunk returns for the same bytes, ordered and rendered in Python by the rules of
`matchy extract` (tests/extract_render_cases.py: line, then the line order of the types, then start; raw bytes; the escapes of the
three formats).

Long candidates: an e-mail with a local part of 600 bytes (854 bytes in all) and a name of nine 63-byte labels (579 bytes) are yielded
whole by the extractor: test_long_candidates_e_mail_and_name sends them through the long tier (above 512 bytes, one wave per candidate)
beside short ones; lengths up to 100 000 bytes and escapes inside long candidates are in tests/test_gpu_extract_render_kernels.py."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

import distinct_cases as D
import extract_render_cases as E

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
MATCHY_ERROR_INVALID_PARAM = -5


@pytest.fixture(scope="module")
def basic():
    import matchy_amd as M
    data = E.library_log()
    ex = M.Extractor(M.EXTRACT_ALL)
    cands = E.candidates(ex, data)
    want = {fmt: E.block(data, cands, fmt) for fmt in E.FORMATS}
    counts = {}
    for t, _, _ in cands:
        counts[E.TYPE_NAMES[t]] = counts.get(E.TYPE_NAMES[t], 0) + 1
    yield {"data": data, "cands": cands, "want": want, "counts": counts, "ex": ex}
    ex.close()


def test_log_has_what_the_case_is_about(basic):
    data, cands = basic["data"], basic["cands"]
    assert {t for t, _, _ in cands} == set(range(12))          # every item type
    assert 2000 <= data.count(b"\n") <= 6000 and len(cands) > 4000
    assert b"\r\n" in data and not data.endswith(b"\n") and b"\x0c" in data
    lines = {data.count(b"\n", 0, s) for _, s, _ in cands}
    assert len(lines) < len(cands)                               # lines with several candidates: the rank decides


@pytest.mark.parametrize("fmt", list(E.FORMATS))
def test_block_and_counts(basic, fmt):
    text, counts = basic["ex"].extract_rendered(basic["data"], fmt)
    assert counts == basic["counts"]
    assert text == basic["want"][fmt]


def test_pieces_of_scan_host_are_joined(basic):
    env = dict(os.environ, MATCHY_AMD_HOST_PIECE_BYTES=str(16 << 10))
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "extract_render_cases.py"), "pieces"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    got = json.loads(p.stdout)
    assert len(basic["data"]) > 10 * (16 << 10)                  # more than ten pieces
    for fmt in E.FORMATS:
        assert got[fmt]["counts"] == basic["counts"]
        assert bytes.fromhex(got[fmt]["text"]) == basic["want"][fmt]


def test_unique_over_two_calls_and_after_reset(basic):
    import matchy_amd as M
    chunks = D.cut(basic["data"], 2)
    model, ex = M.Extractor(M.EXTRACT_ALL, unique=True), M.Extractor(M.EXTRACT_ALL, unique=True)
    try:
        firsts = []
        for k, ch in enumerate(chunks):
            cands = E.candidates(model, ch)                       # exactly what extract_chunk returns with the set on
            assert cands and len(cands) < len(E.candidates(basic["ex"], ch))   # values repeat, inside a call and across the two
            fmt = ("json", "csv")[k]
            text, counts = ex.extract_rendered(ch, fmt)
            assert text == E.block(ch, cands, fmt) and sum(counts.values()) == len(cands)
            assert ex.unique_count == model.unique_count
            firsts.append((cands, text))
        assert ex.extract_rendered(chunks[0], "text") == (b"", {})   # everything seen
        ex.reset_unique()
        text, _ = ex.extract_rendered(chunks[0], "json")
        assert text == firsts[0][1]
        # the set is the handle's whichever entry fills it: extract_chunk behind extract_rendered finds nothing new
        assert ex.extract_from_chunk(chunks[0]) == []
    finally:
        model.close(); ex.close()


def test_empty_buffer_and_buffer_without_candidates(basic):
    ex = basic["ex"]
    for fmt in E.FORMATS:
        assert ex.extract_rendered(b"", fmt) == (b"", {})
        assert ex.extract_rendered(b"GET ok from\n\n  \r\nnothing here\n", fmt) == (b"", {})


def test_invalid_parameters(basic):
    import matchy_amd as M
    L, h = M.lib(), basic["ex"]._h
    out = M._ExtractText()
    assert L.matchy_amd_extractor_extract_rendered(None, b"x", 1, 0, C.byref(out)) == MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_amd_extractor_extract_rendered(h, b"x", 1, 0, None) == MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_amd_extractor_extract_rendered(h, None, 1, 0, C.byref(out)) == MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_amd_extractor_extract_rendered(h, b"x", 1, 3, C.byref(out)) == MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_amd_extractor_extract_rendered(h, None, 0, 2, C.byref(out)) == 0 and out.text_len == 0 and out.n_records == 0
    # the handle still works, and extract_chunk is what it was
    assert E.candidates(basic["ex"], basic["data"]) == basic["cands"]


def test_second_call_regrows_no_buffer(basic):
    import matchy_amd as M
    ex = M.Extractor(M.EXTRACT_ALL)
    try:
        assert ex.render_allocations == 0                        # nothing of the pass exists before its first use
        ex.extract_from_chunk(basic["data"])
        assert ex.render_allocations == 0
        first = ex.extract_rendered(basic["data"], "json")
        n = ex.render_allocations
        assert n > 0
        assert ex.extract_rendered(basic["data"], "json") == first and ex.render_allocations == n
        assert ex.extract_rendered(basic["data"], "text")[0] == basic["want"]["text"] and ex.render_allocations == n
        ms = ex.render_timing()
        assert len(ms) == 4 and all(m >= 0 for m in ms) and ms[0] > 0
    finally:
        ex.close()


def test_long_candidates_e_mail_and_name(basic):
    """an e-mail of 854 bytes and a name of 579 bytes go through the long tier, between short candidates of their lines"""
    label = b"a" * 63
    name = b".".join([label] * 3 + [b"b" * 57]) + b".com"           # 253 bytes
    long_name = b".".join([label] * 9) + b".com"                     # 579 bytes
    data = b"x " + name + b" y 10.0.0.7\n" + b"u" * 600 + b"@" + name + b" z 10.0.0.8\n" + long_name + b" 10.0.0.9\n" + b"f" * 700 + b"\n"
    cands = E.candidates(basic["ex"], data)
    lengths = sorted(e - s for _, s, e in cands)
    assert lengths[-2:] == [len(long_name), 600 + 1 + len(name)] and lengths[-2] > 512 and lengths[0] <= 512
    for fmt in E.FORMATS:
        text, counts = basic["ex"].extract_rendered(data, fmt)
        assert text == E.block(data, cands, fmt) and sum(counts.values()) == len(cands)
