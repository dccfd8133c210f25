"""GPU (-m gpu): the IPv6 path with constructed input — k_anchor's "::" anchors, val_ipv6 / val_ipv6_win, d_parse_ipv6, the
128-level walk trie_v6, and both tree-version quirks with the IPv4 tables built from a start node that is not the root —
against the oracle AND against the Python models of tests/ipv6_cases.py (test_ipv6_host.py holds the two against each other
on the CPU). Every buffer is at most 256 KB; floors and hit counts come from the models."""
import ipaddress
import json
import os
import random
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ipv6_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EX_IPV6 = 1 << 3


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


@pytest.fixture(scope="module")
def ex(M):
    e = M.Extractor()
    yield e
    e.close()


def _build(M, entries, epoch=1700000000):
    b = M.DatabaseBuilder(build_epoch=epoch)
    for k, v in entries:
        b.add_entry(k, v)
    blob = b.build()
    b.close()
    return blob


def _check_extract(ex, oracle, buf, what):
    """GPU == oracle on every item, and the IPv6 items == the model"""
    assert len(buf) <= 256 * 1024
    got = ex.extract_from_chunk(buf)
    assert got == oracle.extract(buf), what
    assert C.packed_items(got) == C.model_extract(buf), what
    return got


# ------------------------------------------------------------------------------------------------ (a) extraction fuzz
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ipv6_extraction_fuzz(M, ex, oracle, seed):
    buf, toks = C.token_corpus(seed)
    got = _check_extract(ex, oracle, buf, seed)
    v6 = [it for it in got if it[0] == "IPv6"]
    rest = [it for it in got if it[0] != "IPv6"]
    assert len(C.accepted_tokens(buf, toks)) >= len(toks) // 10 and rest
    only = M.Extractor(flags=EX_IPV6)
    assert only.extract_from_chunk(buf) == v6 == oracle.extract(buf, flags=EX_IPV6)
    only.close()
    without = M.Extractor(flags=M.EXTRACT_ALL & ~EX_IPV6)
    assert without.extract_from_chunk(buf) == rest == oracle.extract(buf, flags=M.EXTRACT_ALL & ~EX_IPV6)
    without.close()


# ------------------------------------------------------------------------------------------------ (b) window and buffer edges
def _run(k):
    """a hex-and-colon run of k bytes that starts and ends with a hex digit and holds no "::" """
    r = (b"1a2b:3C4d:5e6F:7081:92A3:b4c5:D6e7:f809:0a1B:" * 2)[:k]
    return r[:-1] + b"9" if r.endswith(b":") else r


T35 = b"1a2b:3C4d:5e6F::7081:92A3:b4c5:D6e7"      # the longest text that parses
T8, T7, TFE = b"1::2:345", b"1::2:34", b"fe9A::1:2:3"
LONG = ([_run(38) + b"::" + _run(39),              # "::" at buffer offset 39: 79 bytes on the path that reads the log directly
         _run(40) + b"::7081:92A3"]                # 40 bytes in front of a tail that would parse
        + [_run(k) + b"::1:2" for k in (38, 39, 41)] + [b"1:2::" + _run(k) for k in (38, 39, 40, 41)])
EDGE_TOKENS = [T35, T8, T7, TFE] + LONG


def _edge_buffers():
    """(what, buffer): the second ':' of each token's "::" at every offset 1..45 from the start and at every distance 1..45
    from the end of a buffer; the token is cut where it does not fit, padded with a delimiter ('z') or with more of a run ('7')
    where it does. The far side is long enough for the window path (40 bytes on either side of the anchor)."""
    assert len(T35) == 35 and len(T8) == 8 and len(T7) == 7 and [len(t.split(b"::")[0]) for t in LONG[:2]] == [38, 40]
    for tok in EDGE_TOKENS:
        d = tok.index(b"::") + 1                      # the second ':' inside the token
        after = len(tok) - d - 1
        for off in range(1, 46):
            for pad in (b"z", b"7"):
                head = tok[d - off:] if off < d else pad * (off - d) + tok
                buf = head + b" " + b"z" * 64
                assert buf[off - 1:off + 1] == b"::"
                yield (tok, "start", off, pad), buf
                room = off - 1                         # bytes behind the second ':'
                tail = tok[:d + 1 + room] if room < after else tok + pad * (room - after)
                buf = b"z" * 64 + b" " + tail
                assert buf[len(buf) - off - 1:len(buf) - off + 1] == b"::"
                yield (tok, "end", off, pad), buf


def test_ipv6_buffer_start_and_end(ex, oracle):
    n = accepted = 0
    for what, buf in _edge_buffers():
        accepted += len(_check_extract(ex, oracle, buf, what))
        n += 1
    assert n == len(EDGE_TOKENS) * 45 * 4
    # the accepted tokens fit whole behind 'z' padding at offsets 15..45 / 2..45 from the start and 20..45 / 6..45 from the end
    # (many of their cut and fused forms parse too)
    assert accepted >= 31 + 44 + 26 + 40


def test_ipv6_tokens_straddle_row_block_and_segment_edges(ex, oracle):
    """each accepted token across the 64 B, 1 KiB, 16 KiB and 32 KiB edges at every shift; one buffer holds one shift at all
    four edges, lines of padding between them"""
    for tok in (T35, T8):
        for shift in range(0, len(tok) + 2):
            buf = bytearray()
            for edge in (64, 1024, 16384, 32768):
                start = edge - shift
                fill = start - 1 - len(buf)
                buf += (b"padding line\n" * (fill // 13 + 1))[-fill:] if fill > 0 else b""
                buf += b" " + tok + b" tail\n"
                assert buf[start:start + len(tok)] == tok
            got = _check_extract(ex, oracle, bytes(buf), (tok, shift))
            assert len(got) == 4


# ------------------------------------------------------------------------------------------------ (c) shapes
def test_ipv6_shape_tokens(ex, oracle):
    got = _check_extract(ex, oracle, C.shape_buffer(), "shapes")
    assert len([it for it in got if it[0] == "IPv6"]) >= 44 * 2   # each accepted shape between spaces and between brackets at least


# ------------------------------------------------------------------------------------------------ scans
def _scan_checked(M, oracle, blob, text):
    """_scan_both (host entry, forked, sliced, submitted, compact): everything equals the oracle. -> {(start, end): (type,
    prefix_len, data)} of the IP hits, the data taken from the rendered record of the hit"""
    from tests.test_gpu_parity import _scan_both
    assert len(text) <= 256 * 1024
    gh, gl, gs, wh, wl, ws = _scan_both(M, oracle, blob, text)
    assert gs == ws
    assert gh == wh
    assert gl == wl
    assert len(gl) == len(gh)
    out = {}
    for h, line in zip(gh, gl):
        rec = json.loads(line)
        assert h["kind"] == "ip" and rec["matched_text"].encode() == text[h["start"]:h["end"]] and rec["prefix_len"] == h["prefix_len"]
        out[(h["start"], h["end"])] = (h["type"], h["prefix_len"], rec["data"])
    assert len(out) == len(gh)
    return out, gs


def _v4_spans(oracle, text):
    return [(s, e, int(ipaddress.IPv4Address(v))) for t, s, e, v in oracle.extract(text) if t == "IPv4"]


def _model_hits(oracle, text, v6_lookup, v4_lookup):
    """what the models expect of a scan: IPv6 candidates of model_extract through v6_lookup; IPv4 candidates (the oracle's
    extraction: dotted quads are not this file's subject) through v4_lookup"""
    want = {}
    for s, e, packed in C.model_extract(text):
        r = v6_lookup(int.from_bytes(packed, "big"))
        if r is not None:
            want[(s, e)] = ("IPv6", r[0], r[1])
    for s, e, a in _v4_spans(oracle, text):
        r = v4_lookup(a)
        if r is not None:
            want[(s, e)] = ("IPv4", r[0], r[1])
    return want


@pytest.fixture(scope="module")
def trie_case():
    case = C.trie_case(1)
    case["model"] = C.TrieModel(case["entries"] + case["v4_entries"])
    return case


# ------------------------------------------------------------------------------------------------ (d) IPv6 tree, IPv4 inside
@pytest.mark.parametrize("bits,l24", [(24, None), (24, "0"), (28, None), (32, None)])
def test_ipv6_tree_with_ipv4_inside(M, oracle, monkeypatch, trie_case, bits, l24):
    """3000 IPv4 entries push the tree past 4096 nodes: the /24 table, the leaf tables and the bitmap are built on the device
    from the node behind the 96-zero chain (MATCHY_AMD_L24=0: 16-level table + walk, bitmap from the host)"""
    model, text = trie_case["model"], trie_case["log"]
    monkeypatch.setenv("MATCHY_AMD_MIN_RECORD_SIZE", str(bits))
    blob = _build(M, trie_case["entries"] + trie_case["v4_entries"])
    monkeypatch.delenv("MATCHY_AMD_MIN_RECORD_SIZE")
    meta = oracle.Database(blob).metadata()
    assert meta["ip_version"] == 6 and meta["record_size"] == bits and meta["node_count"] > 4096
    want = _model_hits(oracle, text, model.lookup, model.v4_lookup)
    v6 = [w for w in want.values() if w[0] == "IPv6"]
    assert len(v6) >= 300 and len(want) - len(v6) >= 100
    for lo, hi in ((1, 16), (17, 64), (65, 127), (128, 128)):
        assert any(lo <= w[1] <= hi for w in v6), (lo, hi)
    assert sum(1 for w in v6 if w[1] > w[2]["p"]) >= 50     # the depth of the record, not the entry's prefix
    if l24 is not None:
        monkeypatch.setenv("MATCHY_AMD_L24", l24)
    got, _ = _scan_checked(M, oracle, blob, text)
    assert got == want


def _query_child(blob, qs, tmp_path):
    """the same queries through the lookup KERNELS (MATCHY_AMD_QUERY_ON_GPU=1) in a child process -> [[found, list]]"""
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


def test_ipv6_single_queries_host_path_and_kernels(M, oracle, trie_case, tmp_path):
    """200 probes through Database.lookup and query_json (host walk) and through the lookup kernels: the model's answers"""
    model = trie_case["model"]
    blob = _build(M, trie_case["entries"] + trie_case["v4_entries"])
    rng = random.Random(11)
    qs = rng.sample(trie_case["probes"], 150)
    qs = [rng.choice(C.spellings(q) or [q]) for q in qs[:75]] + qs[75:] + rng.sample(trie_case["v4_written"], 50)
    want = []
    for q in qs:
        a = ipaddress.ip_address(q)
        want.append(model.lookup(int(a)) if a.version == 6 else model.v4_lookup(int(a)))
    assert sum(w is not None for w in want) >= 150 and sum(w is None for w in want) >= 5
    db, odb = M.Database(blob), oracle.Database(blob)
    host = []
    for q, w in zip(qs, want):
        o = odb.lookup(q)
        assert ((o["prefix_len"], o["data"]) if o["kind"] == "ip" else None) == w, q
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


# ------------------------------------------------------------------------------------------------ (e) IPv6-only tree
V6_ONLY = [("2001:db8::/32", {"n": 0}), ("1:8000::/20", {"n": 1}), ("1:4000:1200::/40", {"n": 2}), ("1:c0de::/32", {"n": 3}),
           ("1:2000:0:7::/64", {"n": 4}), ("8000:1::/32", {"n": 5}), ("c000::/8", {"n": 6}), ("a000:0:5::/48", {"n": 7}),
           ("6000::/3", {"n": 8}), ("100::/16", {"n": 9}), ("10:2::/40", {"n": 10}), ("4000:0:0:1::/64", {"n": 11}),
           ("3ffe::/16", {"n": 12}), ("800::/5", {"n": 13}), ("1:1234:5600::/40", {"n": 14})]


@pytest.mark.parametrize("l24", [None, "1"])
def test_ipv6_only_tree_answers_ghost_ipv4(M, oracle, monkeypatch, l24):
    """tree.rs:258-277: without IPv4 entries the 96-zero chain ends a few levels deep and IPv4 bits are read from there; the
    first-level table and the bitmap (host) or the /24 and leaf tables (MATCHY_AMD_L24=1: on the device) start at that node"""
    model = C.TrieModel(V6_ONLY)
    d = model.v4_chain_depth()
    ghosts = model.ghost_v4()
    assert d == 15 and len(ghosts) >= 4
    rng = random.Random(5)
    text = bytearray()
    for k, (lo, hi) in enumerate(ghosts):
        for a in (lo - 1, lo, rng.randint(lo, hi), hi, hi + 1):
            text += b"from " + str(ipaddress.IPv4Address(a & 0xFFFFFFFF)).encode() + rng.choice([b" ", b",", b"\n"])
        text += b"\n"
    for _ in range(300):
        text += str(ipaddress.IPv4Address(rng.getrandbits(32))).encode() + rng.choice([b" ", b"\n"])
    for key, _ in V6_ONLY:
        net = ipaddress.ip_network(key)
        for a in (int(net.network_address) + 1, int(net.network_address) - 1, int(net.broadcast_address) - 1):
            for t in C.spellings(a)[:2]:
                text += b" [" + t.encode() + b"]\n"
    text += b"padding to the end of the buffer " * 3 + b"\n"
    text = bytes(text)
    blob = _build(M, V6_ONLY)
    meta = oracle.Database(blob).metadata()
    assert meta["ip_version"] == 6 and meta["node_count"] < 4096
    want = _model_hits(oracle, text, model.lookup, model.v4_in_v6only)
    n_v4 = sum(1 for w in want.values() if w[0] == "IPv4")
    assert n_v4 >= 3 * len(ghosts) and len(want) - n_v4 >= 10
    # the neighbours just outside the narrow ghost ranges are in the log and expected to miss
    spans = {a: (s, e) for s, e, a in _v4_spans(oracle, text)}
    lo, hi = min(ghosts, key=lambda r: r[1] - r[0])
    assert spans[lo] in want and spans[hi] in want and spans[lo - 1] not in want and spans[hi + 1] not in want
    if l24 is not None:
        monkeypatch.setenv("MATCHY_AMD_L24", l24)
    got, _ = _scan_checked(M, oracle, blob, text)
    assert got == want


# ------------------------------------------------------------------------------------------------ (f) IPv4-only tree
@pytest.mark.parametrize("count", [40, 3000])
def test_ipv4_tree_answers_ipv6_candidates(M, oracle, count):
    """An IPv4 tree answers an IPv6 candidate from its first 32 bits; candidates whose /24 holds nothing are dropped by the
    bitmap pre-filter but still counted. 40 entries: bitmap from the host; 3000: k_ip_l24 builds it."""
    entries = C.v4_entries(3, count)
    model = C.TrieModelV4(entries)
    rng = random.Random(count)
    nets = [ipaddress.ip_network(k) for k, _ in entries]
    occupied = set()       # /24 prefixes that hold an entry or lie inside one
    for n in nets:
        first, last = int(n.network_address) >> 8, int(n.broadcast_address) >> 8
        if last - first < 70000:
            occupied.update(range(first, last + 1))
    wide = [n for n in nets if n.prefixlen < 16]

    def token(a32):
        g = [a32 >> 16, a32 & 0xFFFF] + [rng.choice([0, 0, rng.getrandbits(16)]) for _ in range(5)] + [rng.getrandbits(16) | 1]
        g[rng.randint(2, 6)] = 0
        a = 0
        for v in g:
            a = (a << 16) | v
        forms = [t for t in C.spellings(a) if C.extractable(t)]
        return rng.choice(forms).encode()

    text = bytearray(b"ipv6 candidates against an ipv4 tree\n")
    empty24 = []
    for n in rng.sample(nets, 40):
        lo, hi = int(n.network_address), int(n.broadcast_address)
        for a in (lo, hi, rng.randint(lo, hi), lo - 1, hi + 1):
            if (a >> 24) not in (0, 0xfe) and 0 <= a <= 0xFFFFFFFF:
                text += b"src=" + token(a) + rng.choice([b" ", b"\n", b";"])
        while True:
            v = rng.getrandbits(24)
            if v >> 16 not in (0, 0xfe) and v not in occupied and not any(ipaddress.ip_address(v << 8) in w for w in wide):
                break
        a = (v << 8) | rng.getrandbits(8)
        empty24.append(a)
        text += b" dst=" + token(a) + b"\n"
    text = bytes(text)
    want = _model_hits(oracle, text, model.v6_in_v4tree, model.lookup)
    cands = C.model_extract(text)
    unlisted = [p for s, e, p in cands if int.from_bytes(p[:4], "big") in empty24]
    assert len(want) >= 40 and len(unlisted) == len(empty24) == 40
    assert all(model.v6_in_v4tree(int.from_bytes(p, "big")) is None for p in unlisted)
    blob = _build(M, entries)
    meta = oracle.Database(blob).metadata()
    assert meta["ip_version"] == 4 and (meta["node_count"] < 4096) == (count == 40)
    got, stats = _scan_checked(M, oracle, blob, text)
    assert got == want
    assert stats[1] >= len(cands)       # the dropped candidates are counted (the counters equal the oracle's: _scan_checked)
