"""GPU: distinct candidate texts on the device (csrc/distinct.hip, matchy_amd_extractor_set_unique / `Extractor(unique=True)`).

The model is plain Python (tests/distinct_cases.py): the same handle class with unique off, its output walked in order with a set() of
data[start:end]; what is expected is the entries whose text was not in the set yet, compared as whole (item_type, start, end, value)
entries in order — so the feature is checked against the existing, oracle-pinned extractor."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distinct_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = D.ROOT


@pytest.fixture(scope="module")
def basic():
    """The basic log, the plain extractor's output for it and the model's — computed once, never modified."""
    import matchy_amd as M
    data = D.basic_log()
    ex = M.Extractor(M.EXTRACT_ALL)
    plain = [list(x) for x in ex.extract_from_chunk(data)]
    ex.close()
    seen = set()
    want = D.first_occurrences(plain, data, seen)
    return {"data": data, "plain": plain, "want": want, "seen": seen}


def _child(case, env):
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "distinct_cases.py"), case], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout)


def test_basic_log_has_what_the_case_is_about(basic):
    data, plain, seen = basic["data"], basic["plain"], basic["seen"]
    assert 200 << 10 <= len(data) <= 320 << 10
    assert 3500 <= len(plain) and 250 <= len(seen) <= 400
    classes = {"IPv6", "IPv4", "Email", "Domain", "Bitcoin", "Ethereum", "Monero"}
    types = {t for t, _, _, _ in plain}
    assert classes <= types and types & {"MD5", "SHA1", "SHA256", "SHA384", "SHA512"}, types
    texts = [data[s:e] for _, s, e, _ in plain]
    assert texts.count(b"10.0.0.1") > 2000
    assert {b"host1.example.com", b"Host1.Example.com", b"HOST1.example.com", b"a.example.com", b"aa.example.com", b"2001:db8::a", b"2001:DB8::A"} <= seen
    assert any(t.isupper() and t.lower() in seen for t in seen if len(t) == 32)   # an MD5 in both cases


def test_basic_equals_the_model(basic):
    got, counts = D.run_chunks([basic["data"]], True)
    assert got == basic["want"]
    assert counts == [len(basic["seen"])]
    assert len(got) < len(basic["plain"]) // 8


def test_three_chunks_equal_the_model_over_the_concatenation(basic):
    chunks = D.cut(basic["data"], 3)
    got, counts = D.run_chunks(chunks, True)
    want, want_counts = D.model_chunks(chunks)
    assert got == want and counts == want_counts
    # what stays of a text is its first occurrence in the whole log, whichever chunk holds it
    assert sorted(basic["data"][s:e] for _, s, e, _ in got) == sorted(basic["seen"])
    assert counts[-1] == len(basic["seen"])


def test_pieces_of_scan_host_share_the_set(basic):
    r = _child("pieces", {"MATCHY_AMD_HOST_PIECE_BYTES": str(16 << 10)})
    assert r["got"] == basic["want"]
    assert r["got_counts"] == [len(basic["seen"])]


def test_reset_repeats_the_first_chunk_and_restarts_the_count(basic):
    import matchy_amd as M
    chunks = D.cut(basic["data"], 3)
    ex = M.Extractor(M.EXTRACT_ALL, unique=True)
    first = ex.extract_from_chunk(chunks[0])
    n_first = ex.unique_count
    assert first and ex.extract_from_chunk(chunks[0]) == [] and ex.unique_count == n_first
    ex.extract_from_chunk(chunks[1])
    assert ex.unique_count > n_first
    ex.reset_unique()
    assert ex.unique_count == 0 and ex.unique
    assert ex.extract_from_chunk(chunks[0]) == first and ex.unique_count == n_first
    ex.close()


def test_growth_of_table_and_pool_with_live_entries():
    data, n = D.CASES["growth"]()
    chunks = D.cut(data, n)
    want, want_counts = D.model_chunks(chunks)
    assert want_counts[-1] >= 5000 and all(b - a > 500 for a, b in zip([0] + want_counts, want_counts))
    # 64 slots and 1 KiB of pool against 5 000 texts of ~100 KiB: the table is rehashed and the pool regrown in every chunk
    r = _child("growth", {"MATCHY_AMD_DISTINCT_SLOTS": "64", "MATCHY_AMD_DISTINCT_POOL_BYTES": "1024"})
    assert r["got"] == want and r["got_counts"] == want_counts


@pytest.mark.parametrize("case,bits,n_texts", [("collide4", 4, 500), ("collide0", 0, 64)])
def test_forced_hash_collisions(case, bits, n_texts):
    data, n = D.CASES[case]()
    chunks = D.cut(data, n)
    want, want_counts = D.model_chunks(chunks)
    assert want_counts[-1] >= n_texts and want_counts[0] > n_texts // 4   # many of them new in the same batch
    r = _child(case, {"MATCHY_AMD_DISTINCT_HASH_BITS": str(bits)})
    assert r["got"] == want and r["got_counts"] == want_counts


def test_off_means_off(basic):
    import matchy_amd as M
    ex = M.Extractor(M.EXTRACT_ALL)
    assert not ex.unique and ex.unique_count == 0
    assert [list(x) for x in ex.extract_from_chunk(basic["data"])] == basic["plain"]
    ex.set_unique(True)
    ex.set_unique(False)
    assert not ex.unique
    assert [list(x) for x in ex.extract_from_chunk(basic["data"])] == basic["plain"]
    # switched on behind that, the set starts empty: unique-off calls add nothing to it
    ex.set_unique(True)
    assert [list(x) for x in ex.extract_from_chunk(basic["data"])] == basic["want"]
    ex.close()


def test_empty_and_degenerate_chunks():
    import matchy_amd as M
    ex = M.Extractor(M.EXTRACT_ALL, unique=True)
    assert ex.extract_from_chunk(b"") == [] and ex.unique_count == 0
    assert ex.extract_from_chunk(b"no candidate in here\njust words\n") == [] and ex.unique_count == 0
    line = b"x 192.0.2.77 y\n"
    got = ex.extract_from_chunk(line * 1000)
    assert got == [("IPv4", 2, 12, "192.0.2.77")] and ex.unique_count == 1
    assert ex.extract_from_chunk(b"") == [] and ex.extract_from_chunk(line) == [] and ex.unique_count == 1
    ex.close()
