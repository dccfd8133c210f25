"""GPU (-m gpu): IPv4, e-mail, domain and hash extraction (k_anchor's patterns and drains, k_validate_dom, val_domain_ctx /
val_email_ctx, the long-token trigger), the scan's lookups of those candidates, and the IPv4 tables (ip_l1, ip_l24 / ip_bm24 /
ip_leaf in their four variants) against the Python models of tests/extract_cases.py and TrieModelV4 — not against oracle/
(test_extract_model_host.py holds the models against the oracle and the reference's vectors on the CPU). Every buffer is at most
256 KB; floors and hit counts come from the models and the entry lists."""
import ipaddress
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import extract_cases as E   # noqa: E402
import ipv6_cases as C6     # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


@pytest.fixture(scope="module")
def extractors(M):
    exs = {s: M.Extractor(flags=s[0], min_domain_labels=s[1]) for s in E.SETTINGS}
    yield exs
    for e in exs.values():
        e.close()


_cache = {}


def corpus(kind, seed):
    if (kind, seed) not in _cache:
        _cache[(kind, seed)] = E.CORPORA[kind](seed)
    return _cache[(kind, seed)]


# ------------------------------------------------------------------------------------------------ extraction
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", ["ipv4", "email", "domain", "hash"])
def test_extraction_equals_model_on_corpus(extractors, kind, seed):
    """spans, types and values, at every setting"""
    buf, toks = corpus(kind, seed)
    assert len(buf) <= 256 * 1024
    for (flags, min_labels), ex in extractors.items():
        assert E.four(ex.extract_from_chunk(buf)) == E.model(buf, flags, min_labels), (kind, seed, flags, min_labels)
    print(f"{kind} corpus {seed}: {len(toks)} tokens, {len(E.model(buf))} items, {len(E.SETTINGS)} settings")


@pytest.fixture(scope="module")
def edge_buffers():
    return E.place_on_edges(E.edge_tokens())


@pytest.mark.parametrize("setting", E.SETTINGS, ids=lambda s: f"flags{s[0]}-labels{s[1]}")
def test_extraction_equals_model_on_edge_buffers(extractors, edge_buffers, setting):
    """every byte of every token on the row (256), block (2048, 2048 + 256, 6144), window / segment (8192, 16384) edges of
    k_anchor, and on the first and last byte of a buffer"""
    ex = extractors[setting]
    items = 0
    for what, buf in edge_buffers:
        want = E.model(buf, *setting)
        assert E.four(ex.extract_from_chunk(buf)) == want, (what, setting)
        items += len(want)
    assert items > 0
    print(f"edge buffers at {setting}: {len(edge_buffers)} buffers of {len(E.edge_tokens())} tokens, {items} items")


def test_extraction_equals_model_on_buffer_tails(extractors):
    for body in E.ipv4_tail_cases():
        for setting, ex in extractors.items():
            assert E.four(ex.extract_from_chunk(body)) == E.model(body, *setting), (body, setting)


# ------------------------------------------------------------------------------------------------ scans
def _build(M, entries, epoch=1700000000, case_insensitive=False):
    b = M.DatabaseBuilder(build_epoch=epoch, case_insensitive=case_insensitive)
    for k, v in entries:
        b.add_entry(k, v)
    blob = b.build()
    b.close()
    return blob


def _scan_all_entries(M, blob, text):
    """Scanner.scan, then the same bytes through the device-resident entries (forked, 2 / 3 / 5 slices cut at 8 KiB multiples,
    submitted, compact records), which must give the same records -> (hits, ndjson lines, (lines, candidates))"""
    from tests.test_gpu_parity import _device_entries
    assert len(text) <= 256 * 1024
    db = M.Database(blob)
    sc = M.Scanner(db)
    res = sc.scan(text)
    hits, lines, stats = res.hits(), res.ndjson(text, source="t.log"), (res.lines, res.candidates)
    res.close()
    _device_entries(sc, text, hits, lines, stats, slices=(2, 3, 5))
    sc.close()
    db.close()
    return hits, lines, stats


@pytest.fixture(scope="module")
def scan_case():
    case = E.scan_case(1)
    case["trie"] = C6.TrieModelV4(case["v4"])
    return case


@pytest.mark.parametrize("case_insensitive", [False, True], ids=["exact", "folded"])
@pytest.mark.parametrize("kind", ["ipv4", "email", "domain", "hash"])
def test_scan_hits_equal_model(M, scan_case, kind, case_insensitive):
    """(start, end, type, prefix length) of every hit and the candidate count, from the models alone"""
    blob = _build(M, scan_case["entries"], epoch=7, case_insensitive=case_insensitive)
    buf, _ = corpus(kind, 1)
    want, cands = E.model_hits(buf, scan_case["keys"], scan_case["trie"], case_insensitive)
    assert len(want) >= 100
    hits, _, stats = _scan_all_entries(M, blob, buf)
    assert sorted((h["start"], h["end"], h["type"], h["prefix_len"]) for h in hits) == want
    assert all((h["kind"] == "ip") == (h["type"] == "IPv4") for h in hits)
    assert stats[1] == cands
    print(f"scan of the {kind} corpus ({'folded' if case_insensitive else 'exact'}): {cands} candidates, {len(want)} hits")


# ------------------------------------------------------------------------------------------------ IPv4 tables
def _query_child(blob, qs, tmp_path):
    """single queries through the lookup KERNELS (MATCHY_AMD_QUERY_ON_GPU=1) in a child process -> [[found, list]]"""
    (tmp_path / "db.mxy").write_bytes(blob)
    (tmp_path / "q.json").write_text(json.dumps(qs))
    code = r"""
import json, sys
sys.path.insert(0, %r)
import matchy_amd as M
db = M.Database(open(sys.argv[1], "rb").read())
json.dump([list(db.query_json(q)) for q in json.load(open(sys.argv[2]))], open(sys.argv[3], "w"))
""" % str(ROOT)
    p = subprocess.run([sys.executable, "-c", code, str(tmp_path / "db.mxy"), str(tmp_path / "q.json"), str(tmp_path / "out.json")],
                       env=dict(os.environ, MATCHY_AMD_QUERY_ON_GPU="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads((tmp_path / "out.json").read_text())


_table_cache = {}


def _table_case(wide):
    if wide not in _table_cache:
        case = E.v4_table_case(1, wide)
        case["model"] = C6.TrieModelV4(case["entries"])
        case["stats"] = E.v4_stats(case["entries"])
        _table_cache[wide] = case
    return _table_cache[wide]


@pytest.mark.parametrize("env", [None, ("MATCHY_AMD_L24", "0"), ("MATCHY_AMD_L24", "1"), ("MATCHY_AMD_LEAF_MB", "0"), ("MATCHY_AMD_LEAF_MB", "1")],
                         ids=lambda e: "default" if e is None else f"{e[0][11:]}={e[1]}")
@pytest.mark.parametrize("wide", [True, False], ids=["wide", "narrow"])
def test_ipv4_tables_equal_trie_model(M, monkeypatch, tmp_path, wide, env):
    """Every prefix length, the nested chain, the ballot-word edges of k_ip_l24 and more deep /24s than MATCHY_AMD_LEAF_MB=1 has
    leaf tables for. wide: more than 250 per mille of the /24s are occupied, so the dense candidate list and k_lookup_ip run;
    narrow: the lookups run inside k_anchor. Hits, prefix lengths and data through scan, scan_device and single queries."""
    case = _table_case(wide)
    model, text = case["model"], case["text"]
    nodes, permille, deep = case["stats"]
    assert nodes >= 4096 and deep > 512 and (permille > 250) == wide          # 2^20 / 2048 = 512 leaf tables at LEAF_MB=1
    assert {d["p"] for _, d in case["entries"]} == set(range(1 if wide else 9, 33))
    want = {}
    for s, e in E.model_ipv4(text):
        r = model.lookup(int(ipaddress.IPv4Address(text[s:e].decode())))
        if r is not None:
            want[(s, e)] = r
    assert len(want) > 1000 and len(E.model_ipv4(text)) - len(want) > (50 if wide else 500)
    assert sum(1 for p, d in want.values() if p > d["p"]) > 100                # the depth of the record, not the entry's prefix
    if env is not None:
        monkeypatch.setenv(*env)
    blob = _build(M, case["entries"])
    hits, lines, stats = _scan_all_entries(M, blob, text)
    assert stats[1] == len(E.model_ipv4(text)) == len(case["probes"])
    assert len(lines) == len(hits)
    got = {}
    for h, line in zip(hits, lines):
        rec = json.loads(line)
        assert h["kind"] == "ip" and h["type"] == "IPv4" and rec["matched_text"].encode() == text[h["start"]:h["end"]] and rec["prefix_len"] == h["prefix_len"]
        got[(h["start"], h["end"])] = (h["prefix_len"], rec["data"])
    assert len(got) == len(hits) and got == want
    # single queries: the host walk, and the lookup kernels in a child process
    rng = random.Random(3)
    qs = [str(ipaddress.IPv4Address(a)) for a in rng.sample(case["probes"], 300)]
    db = M.Database(blob)
    host = []
    for q in qs:
        w = model.lookup(int(ipaddress.IPv4Address(q)))
        assert db.lookup(q) == (None if w is None else {"found": True, "prefix_len": w[0], "data": w[1]}), q
        found, arr = db.query_json(q)
        host.append([found, arr])
        if w is None:
            assert not found and arr == [], q
        else:
            assert found and len(arr) == 1 and arr[0]["prefix_len"] == w[0], (q, arr)
            assert {k: v for k, v in arr[0].items() if k not in ("prefix_len", "cidr")} == w[1], (q, arr)
    db.close()
    assert _query_child(blob, qs, tmp_path) == json.loads(json.dumps(host))
    print(f"IPv4 tables {'wide' if wide else 'narrow'} {env}: {len(case['entries'])} entries, {len(case['probes'])} probes scanned, {len(want)} hits, 300 single queries")
