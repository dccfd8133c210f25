"""CPU: the IPv4 / e-mail / domain / hash models of tests/extract_cases.py against the oracle, against the reference's own
vectors (tests/golden/extractor_kat.json, without passing through the oracle) and against themselves with single rules
switched off; TrieModelV4 against builder + oracle at every IPv4 prefix length. The models are written from the reference's
source, not from oracle/: where the two agree here, test_gpu_extract_model.py uses the model as the kernels' reference."""
import ipaddress
import json
from pathlib import Path

import pytest

import extract_cases as E
import ipv6_cases as C6
import matchy_amd as M

GOLD = Path(__file__).parent / "golden"
OTHER_FLAGS = 255 & ~E.FOUR      # IPv6, Bitcoin, Ethereum, Monero


def _agree(oracle, buf, what):
    for flags, min_labels in E.SETTINGS:
        assert E.four(oracle.extract(buf, flags=flags, min_labels=min_labels)) == E.model(buf, flags, min_labels), (what, flags, min_labels)


_corpus_cache = {}


def corpus(kind, seed):
    if (kind, seed) not in _corpus_cache:
        _corpus_cache[(kind, seed)] = E.CORPORA[kind](seed)
    return _corpus_cache[(kind, seed)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("kind", ["ipv4", "email", "domain", "hash"])
def test_model_equals_oracle_on_corpus_and_floors_hold(oracle, kind, seed):
    buf, toks = corpus(kind, seed)
    assert 90_000 <= len(buf) <= 256 * 1024 and b"::" not in buf
    _agree(oracle, buf, (kind, seed))
    # nothing of the other four types: a scan's candidate count over this corpus is the model's item count
    assert oracle.extract(buf, flags=OTHER_FLAGS) == []
    # floors, from the model alone (tune the generator, not the floors)
    items = E.model(buf)
    v = E.verdicts(toks, items)
    assert len(E.accepted(buf, toks)) >= len(toks) // 10
    assert sum(1 for x in v if not x) >= len(toks) // 4
    for model, rule, min_labels in E.RULES[kind]:
        assert E.flips(buf, toks, model, rule, 255, min_labels) >= 50, (model, rule)
    for key in E.UNOBSERVABLE:
        model, rule = key.split(".")
        assert E.model(buf, 255, 2, {model: (rule,)}) == items, key


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ladders_occur_among_the_accepted_tokens(seed):
    buf, toks = corpus("domain", seed)
    front, behind = set(), set()
    for s, e in E.accepted(buf, toks, {"Domain"}):
        for d in E._positions(buf[s:e], b"."):
            front.add(d)
            behind.add(e - s - d)
    assert front >= set(E.DOMAIN_LADDER) and behind >= set(E.DOMAIN_LADDER)
    buf, toks = corpus("email", seed)
    acc = [(buf[s:e].index(b"@"), e - s - 1 - buf[s:e].index(b"@")) for s, e in E.accepted(buf, toks, {"Email"})]
    # an empty local part and a domain part of 3 bytes (the shortest listed form is x.yy) cannot be accepted: they stand among the rejected
    assert {a for a, _ in acc} >= set(E.EMAIL_LOCAL_LADDER) - {0} and {b for _, b in acc} >= set(E.EMAIL_DOMAIN_LADDER) - {3}
    bodies = [buf[s:e] for s, e in toks]
    assert sum(b.startswith(b"@") for b in bodies) >= 50 and sum(b.count(b"@") == 1 and len(b.split(b"@")[1]) == 3 for b in bodies) >= 50
    assert max(a for a, _ in acc) >= 200 and max(b for _, b in acc) >= 100
    buf, toks = corpus("hash", seed)
    acc = E.accepted(buf, toks)
    assert {(e - s, s % 4) for s, e in acc} == {(n, r) for n in E.HASH_TYPES for r in range(4)}
    assert {e - s for s, e in toks} == set(E.HASH_LENGTHS)
    buf, toks = corpus("ipv4", seed)
    assert buf.endswith(b" 9.8.7.6") and (len(buf) - 7, len(buf)) in E.model_ipv4(buf)


@pytest.fixture(scope="module")
def edge_buffers():
    return E.place_on_edges(E.edge_tokens())


def test_model_equals_oracle_on_edge_buffers(oracle, edge_buffers):
    toks = E.edge_tokens()
    assert 40 <= len(toks) <= 60
    placed = set()
    n_items = 0
    for (tok, shift, where), buf in edge_buffers:
        got = E.model(buf)
        assert E.four(oracle.extract(buf)) == got, (tok, shift, where)
        n_items += len(got)
        if isinstance(where, tuple):
            for e in where:
                assert (buf[e:e + 1] == tok[shift:shift + 1]) if 0 <= shift < len(tok) else (buf[e:e + 1] == b" ")
                placed.add((tok, shift, e))
    assert placed == {(t, s, e) for t in toks for s in range(-1, len(t) + 1) for e in E.EDGES}
    assert n_items > len(edge_buffers) // 3
    # the other settings on every seventh buffer (the GPU test runs them all)
    for what, buf in edge_buffers[::7]:
        _agree(oracle, buf, what)
    # each token alone between spaces: the set holds accepted and rejected tokens of every type
    alone = {t: [it for it in E.model(b"- " + t + b" -") if (it[1], it[2]) == (2, 2 + len(t))] for t in toks}
    for typ in (("IPv4",), ("Email",), ("Domain",), tuple(E.HASH_TYPES.values())):
        assert sum(1 for t in toks if alone[t] and alone[t][0][0] in typ) >= 2, typ
    assert sum(1 for t in toks if not alone[t]) >= 25


def test_model_equals_oracle_on_hand_written_inputs(oracle):
    from tests.test_gpu_parity import ADVERSARIAL
    for data in ADVERSARIAL + E.ipv4_tail_cases():
        for buf in (data, b"x " + data + b" y", data + b"\n" + data, b"\n" + data + b"\n"):
            _agree(oracle, buf, buf)


def test_model_equals_oracle_on_alphabet_fuzz(oracle):
    """the 400 buffers of test_extractor_differential_fuzz"""
    import random
    from tests.test_gpu_parity import ALPHABETS
    rng = random.Random(20251212)
    for it in range(400):
        alpha = rng.choice(ALPHABETS)
        n = rng.choice([1, 5, 17, 63, 64, 65, 127, 128, 129, 200, 1000, 1023, 1024, 1025, 5000])
        buf = bytes(rng.choice(alpha) for _ in range(n))
        assert E.four(oracle.extract(buf)) == E.model(buf), (it, buf)
        if it % 16 == 0:
            _agree(oracle, buf, it)


def test_model_gives_the_reference_vectors():
    """tests/golden/extractor_kat.json: the inputs and expected items of the reference's own tests"""
    cases = json.loads((GOLD / "extractor_kat.json").read_text())["cases"]
    checked = 0
    for c in cases:
        data = bytes.fromhex(c["input_hex"]) if "input_hex" in c else c["input"].encode()
        by_type = {}
        for t, s, e, v in E.model(data, c["flags"], c["min_labels"]):
            by_type.setdefault(t, []).append(v)
        for t, want in c["expect"].items():
            if t in E.FOUR_TYPES:
                assert by_type.get(t, []) == want, (c["ref"], t)
                checked += 1
        if "total" in c and all(t in E.FOUR_TYPES for t in c["expect"]) and not c["flags"] & ~E.FOUR & 255:
            assert sum(len(v) for v in by_type.values()) == c["total"], c["ref"]
    assert checked >= 40


def test_psl_decoder():
    s = E.psl()
    assert len(s) > 9000 and b"com" in s and b"co.uk" in s and b"uk" in s and b"*.ck" in s and b"ck" not in s
    assert "рф".encode() in s and b"COM" not in s and not any(k.startswith(b"!") for k in s)
    assert E.find_suffix(b"foo.co.uk") == 6 and E.find_suffix(b"co.uk") == 2 and E.find_suffix(b"com") is None and E.find_suffix(b".com") == 0


def test_models_are_sensitive_to_their_own_rules():
    # IPv4: the count runs over dots[i..] of the whole chunk, not over the run: behind an accepted quad the later dots of a run count
    # the NEXT quad's dots and would parse the same quad again; the cursor is what keeps it single. Alone, the count is enough.
    assert E.model_ipv4(b"1.2.3.4 5.6.7.8") == [(0, 7), (8, 15)]
    assert E.model_ipv4(b"1.2.3.4 5.6.7.8", skip=("cursor",)) == [(0, 7), (0, 7), (0, 7), (8, 15)]
    assert E.model_ipv4(b"1.2.3.4 and more", skip=("cursor",)) == [(0, 7)]
    assert E.model_ipv4(b"1.2.3.4 and more", skip=("cursor", "dots_from_i")) == [(0, 7)] * 3
    assert E.model_ipv4(b"999.1.1.1.1") == [] and E.model_ipv4(b"1.2.3.4.5") == [] and E.model_ipv4(b"999.1.1.1 1.1.1.1") == [(10, 17)]
    assert E.model_ipv4(b"1.2.3.256") == [] and E.model_ipv4(b"1.2.3.256", skip=("le255",)) == [(0, 9)]
    assert E.model_ipv4(b"1.2.3.04") == [] and E.model_ipv4(b"01.2.3.4", skip=("leading_zero",)) == [(0, 8)]
    assert E.model_ipv4(b"x1.2.3.4") == [] and E.model_ipv4(b"1.2.3.4\xff") == [] and E.model_ipv4(b"1.2.3.4:80") == [(0, 7)]
    assert E.model_ipv4(b"1.2.3.1234") == [] and E.model_ipv4(b"1.2.3.1234", skip=("max3",)) == []
    assert E.model_ipv4(b" 1.2.3.4") == [(1, 8)] and E.model_ipv4(b" 1.2.3.") == [] and E.model_ipv4(b"11.2.3") == []
    # e-mail: no cursor, so a chain yields two items that overlap; the domain part is ASCII, so a high byte behind it rejects
    assert E.model_email(b"a@b.com@c.org") == [(0, 7), (2, 13)]
    assert E.model_email(b"u..r@foo.com") == [] and E.model_email(b"u..r@foo.com", skip=("no_dotdot",)) == [(0, 12)]
    assert E.model_email(b"123@foo.com") == [] and E.model_email(b"+1_2@foo.com") == [] and E.model_email(b"1a3@foo.com") == [(0, 11)]
    assert E.model_email(b"u@foo.com\xc3\xa9") == [] and E.model_email(b"u@foo.com\xc3\xa9", skip=("boundary_behind",)) == [(0, 9)]
    assert E.model_email(b"u@foo.123") == [] and E.model_email(b"u@foo") == [] and E.model_email(b"u@foo.com.") == [] and E.model_email(b"u@co.uk") == [(0, 7)]
    assert E.model_email(b"user@@foo.com") == [] and E.model_email(b"!u@foo.com") == [] and E.model_email(b"\xc3\xa9u@foo.com") == []
    # domain: the shortest listed suffix wins, so co.uk is a name under uk; ck is listed only as *.ck, which no name contains
    assert E.model_domain(b"co.uk") == [(0, 5)] and E.model_domain(b"com") == [] and E.model_domain(b".com") == []
    assert E.model_domain(b"foo.ck") == [] and E.model_domain(b"www.ck") == [] and E.model_domain(b"x.www.ck") == []
    assert E.model_domain(b"a.b.com") == [(0, 7)] and E.model_domain(b"a.b.com", skip=("cursor",)) == [(0, 7), (0, 7)]
    # ... only an accept moves the cursor; a cursor that rejects moved too would change nothing, because every dot of a run sees the
    # same candidate (asserted over the corpora: UNOBSERVABLE)
    assert E.model_domain(b"-a.b.com c.d.com") == [(9, 16)] == E.model_domain(b"-a.b.com c.d.com", skip=("accept_only",))
    assert E.model_domain(b"foo.com.") == [] and E.model_domain(b".foo.com") == [] and E.model_domain(b"foo..com") == []
    assert E.model_domain(b"foo-.com") == [] and E.model_domain(b"f-o.com") == [(0, 7)] and E.model_domain(b"foo.-com") == []
    assert E.model_domain(b"foo.com_") == [] and E.model_domain(b"_foo.com") == [] and E.model_domain(b"=foo.com:") == [(1, 8)]
    assert E.model_domain(b"caf\xc3\xa9.fr") == [(0, 8)] and E.model_domain(b"caf\xc3.fr") == [] and E.model_domain(b"a.\xed\xa0\x80.com") == []
    assert E.model_domain(b"\xc0\xafa.com") == [] and E.model_domain(b"\xc0\xafa.com", skip=("utf8",)) == [(0, 7)]
    assert E.model_domain(b"a.com", 1) == [(0, 5)] == E.model_domain(b"a.com", 2) and E.model_domain(b"a.com", 3) == [] and E.model_domain(b"b.a.com", 3) == [(0, 7)]
    assert E.model_domain(b"foo.COM") == [] and E.model_domain(b"FOO.com") == [(0, 7)]
    # hashes: a token is a maximal run of NON-BOUNDARY bytes, so '-', '.', '_' or a letter beside the digits makes it longer
    h = E.H32
    assert E.model_hashes(b"=" + h + b";") == [(1, 33)] and E.model_hashes(b"x" + h) == [] and E.model_hashes(h + b".") == [] and E.model_hashes(h + b"\xff") == []
    assert E.model_hashes(b"x" + h, skip=("boundary",)) == [(1, 33)] and E.model_hashes(h[:-1]) == [] and E.model_hashes(h[:-1] + b"g") == []
    assert E.model_hashes(h[:-1] + b"g", skip=("hex",)) == [(0, 32)] and E.model_hashes(h + b"0") == [] and E.model_hashes(h.upper()) == [(0, 32)]
    # the order of extract_from_chunk: by extractor, not by position
    buf = h + b" u@a.com 1.2.3.4"
    assert [(t, s) for t, s, e, v in E.model(buf)] == [("IPv4", 41), ("Email", 33), ("Domain", 35), ("MD5", 0)]


# ------------------------------------------------------------------------------------------------ IPv4 tables
def _build(entries, epoch=1700000000):
    b = M.DatabaseBuilder(build_epoch=epoch)
    for k, v in entries:
        b.add_entry(k, v)
    blob = b.build()
    b.close()
    return blob


@pytest.mark.parametrize("wide", [True, False])
def test_builder_and_oracle_equal_trie_model_at_every_ipv4_prefix(oracle, wide):
    case = E.v4_table_case(1, wide)
    entries = case["entries"]
    assert {d["p"] for _, d in entries} == set(range(1 if wide else 9, 33))
    nodes, permille, deep = E.v4_stats(entries)
    assert nodes >= 4096 and deep > 512 and (permille > 250) == wide
    # the networks on the ballot-word edges (/24 index 0, 31, 32, 63 modulo 64) have empty neighbours, apart from the wide entries
    held = {}
    for k, d in entries:
        n = ipaddress.ip_network(k)
        if n.prefixlen > 8:
            for v in range(int(n.network_address) >> 8, (int(n.broadcast_address) >> 8) + 1):
                held[v] = held.get(v, 0) + 1
    assert sorted({v % 64 for v in case["ballot"]}) == [0, 31, 32, 63] and len(set(case["ballot"])) == 12
    assert all(held.get(v) == 1 and v - 1 not in held and v + 1 not in held for v in case["ballot"])
    assert all(((v << 8) - 1) in case["probes"] and ((v + 1) << 8) in case["probes"] for v in case["ballot"][::3])   # around the /24 entries
    blob = _build(entries)
    odb = oracle.Database(blob)
    meta = odb.metadata()
    assert meta["ip_version"] == 4 and meta["node_count"] == nodes
    model = C6.TrieModelV4(entries)
    hits = deeper = 0
    for a in case["probes"]:
        want = model.lookup(a)
        f = model.m.formula(a)      # (the model keeps IPv4 entries at depth 96 + p)
        assert want == (f and (f[0] - 96, f[1])), a
        o = odb.lookup(str(ipaddress.IPv4Address(a)))
        assert ((o["prefix_len"], o["data"]) if o["kind"] == "ip" else None) == want, a
        if want is not None:
            hits += 1
            deeper += want[0] > want[1]["p"]
    assert hits > 1000 and deeper > 100 and len(case["probes"]) - hits > (50 if wide else 500)
    # the scan of the oracle over the written probes: (start, end, prefix length) as the models give them
    text = case["text"]
    assert len(text) <= 256 * 1024
    want = {}
    for s, e in E.model_ipv4(text):
        r = model.lookup(int(ipaddress.IPv4Address(text[s:e].decode())))
        if r is not None:
            want[(s, e)] = r[0]
    got, _, st = odb.scan(text, want_json=False)
    assert {(h["start"], h["end"]): h["prefix_len"] for h in got} == want and all(h["type"] == "IPv4" for h in got)
    assert st.candidates == len(E.model_ipv4(text)) == len(case["probes"])


@pytest.mark.parametrize("case_insensitive", [False, True])
def test_scan_expectation_from_the_models_equals_the_oracle_scan(oracle, case_insensitive):
    """what test_gpu_extract_model.py expects of a scan — model items that are keys, TrieModelV4 for the addresses, the candidate
    count — against the oracle's scan of the same database"""
    case = E.scan_case(1)
    b = M.DatabaseBuilder(build_epoch=7, case_insensitive=case_insensitive)
    for k, v in case["entries"]:
        b.add_entry(k, v)
    odb = oracle.Database(b.build())
    b.close()
    trie = C6.TrieModelV4(case["v4"])
    for kind in E.CORPORA:
        buf, _ = corpus(kind, 1)
        want, cands = E.model_hits(buf, case["keys"], trie, case_insensitive)
        got, _, st = odb.scan(buf, want_json=False)
        assert sorted((h["start"], h["end"], h["type"], h["prefix_len"]) for h in got) == want, kind
        assert st.candidates == cands and len(want) >= 100, kind
        if case_insensitive and kind != "ipv4":
            assert len(want) >= len(E.model_hits(buf, case["keys"], trie)[0]) + 30, kind
