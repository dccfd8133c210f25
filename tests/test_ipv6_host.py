"""CPU: the IPv6 models of tests/ipv6_cases.py against the oracle (extraction) and against builder + oracle (the 128-level
walk, both tree-version quirks). The models are written from the reference's sources and from the definition of a
longest-prefix trie, not from oracle/: where the two agree here, test_gpu_ipv6.py may use either as the kernels' reference."""
import ipaddress

import pytest

import ipv6_cases as C
import matchy_amd as M


def _build(entries, epoch=1700000000):
    b = M.DatabaseBuilder(build_epoch=epoch)
    for k, v in entries:
        b.add_entry(k, v)
    blob = b.build()
    b.close()
    return blob


def _ip_answer(w):
    return (w["prefix_len"], w["data"]) if w["kind"] == "ip" else None


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_extraction_model_equals_oracle_on_token_corpus(oracle, seed):
    buf, toks = C.token_corpus(seed)
    assert 150_000 <= len(buf) <= 256 * 1024 and len(toks) == 8000
    want = C.model_extract(buf)
    assert C.packed_items(oracle.extract(buf)) == want
    assert C.packed_items(oracle.extract(buf, flags=1 << 3)) == want
    # floors that keep the corpus from going hollow (tune the generator, not the floors)
    acc = C.accepted_tokens(buf, toks)
    assert len(acc) >= len(toks) // 10
    assert sum(1 for s, e, _ in acc if e - s > 30) >= 20
    assert {pos for _, _, pos in acc} >= {1, 2, 3, 4, 5, 6}
    # look-alikes of every other kind are there too
    bodies = [buf[s:e] for s, e, _ in toks]
    assert sum(b":::" in b for b in bodies) > 300 and sum(b.count(b"::") >= 2 for b in bodies) > 300
    assert sum(b"::" not in b for b in bodies) > 300 and sum(b[:3].lower() in (b"fe8", b"fe9", b"feb") for b in bodies) > 100


def test_extraction_model_equals_oracle_on_shape_tokens(oracle):
    toks = C.shape_tokens()
    buf = C.shape_buffer()
    want = C.model_extract(buf)
    assert C.packed_items(oracle.extract(buf)) == want
    # what the enumeration is there for, decided by the model on each token alone
    alone = {t: C.model_extract(b" " + t + b" ") for t in toks}
    longest = max((t for t in toks if alone[t]), key=len)
    assert len(longest) == 35
    assert alone[b"1::2:345"] and alone[b"12::3:456"] and not alone[b"1::2:34"] and not alone[b"12::3:4"]
    assert alone[b"1a2b:3C4d:5e6F:7081:92A3:b4c5::D6e7"] and not alone[b"1a2b:3C4d:5e6F:7081:92A3:b4c5:D6e7::f809"]   # 7 + "::", 8 + "::"
    assert not alone[toks[-1]] and len(toks[-1]) == 39
    assert not any(alone[t] for t in toks if t.startswith(b"::") or t.endswith(b"::"))
    # inner "::" and 2..7 groups: 21 tokens of 4-digit groups, 18 of 1-digit groups with 4..7 groups (8 bytes and more), 5 extras
    assert sum(1 for t in toks if alone[t]) == 21 + 18 + 5


def test_extraction_model_is_sensitive_to_its_own_rules():
    """case folding of the fe8x filter, and the last_end cursor: every "::" of a run yields the same candidate, so the cursor can
    only show where it overshoots — fused against the next run nothing may be lost, whatever the previous run's verdict"""
    assert C.model_extract(b" FE9a::1:2:3 fE80::1:2:3 FeB0::1:2:3 fec0::1:2:3 ") == [(37, 48, ipaddress.IPv6Address("fec0::1:2:3").packed)]
    want = ipaddress.IPv6Address("1::2:3:4").packed
    for first in (b"1::2::3:4:5", b"a::b", b"::1:2:3:4", b"1:2:3:4::", b"fe80::1:2:3", b"1::2:3:4", b"::", b"g::g"):
        buf = first + b" 1::2:3:4"
        got = C.model_extract(buf)
        assert got[-1] == (len(first) + 1, len(buf), want) and len(got) == 1 + (first == b"1::2:3:4"), first


def test_spellings_cover_every_compressible_run():
    a = ipaddress.IPv6Address("2001:db8:0:0:1:0:0:1")
    forms = C.spellings(a)
    assert "2001:db8::1:0:0:1" in forms and "2001:db8:0:0:1::1" in forms and "2001:db8::0:1:0:0:1" in forms
    assert "2001:0DB8:0000:0000:0001::0001" in forms and len(forms) >= 20
    assert C.spellings(ipaddress.IPv6Address("1:2:3:4:5:6:7:8")) == []
    assert C.spellings(ipaddress.IPv6Address("0:2:3:4:5:6:7:0")) == []      # only leading / trailing "::" possible
    assert C.spellings(ipaddress.IPv6Address("8000::")) and not any(C.extractable(t) and len(t) < 8 for t in C.spellings("8000::"))


@pytest.mark.parametrize("bits", [24, 28, 32])
def test_builder_and_oracle_equal_trie_model(oracle, monkeypatch, bits):
    """every probe of trie_case: prefix length (the depth of the record the walk ends on, not the entry's prefix) and data"""
    case = C.trie_case(1)
    entries = case["entries"] + case["v4_entries"]
    assert {p for p in range(1, 129)} == {d["p"] for _, d in case["entries"]}
    monkeypatch.setenv("MATCHY_AMD_MIN_RECORD_SIZE", str(bits))
    blob = _build(entries)
    monkeypatch.delenv("MATCHY_AMD_MIN_RECORD_SIZE")
    odb = oracle.Database(blob)
    meta = odb.metadata()
    assert meta["record_size"] == bits and meta["ip_version"] == 6 and meta["node_count"] > 4096
    model = C.TrieModel(entries)
    nets = [ipaddress.ip_network(k) for k, _ in case["entries"]]
    hits = deeper = 0
    for q in case["probes"]:
        a = ipaddress.IPv6Address(q)
        want = model.lookup(int(a))
        assert want == model.formula(int(a)), q
        assert _ip_answer(odb.lookup(q)) == want, q
        if any(a in n for n in nets):
            assert want is not None, q     # every probe inside a network hits
        if want is not None:
            hits += 1
            deeper += want[0] > want[1]["p"]
    assert hits > 900 and deeper > 100
    v4_hits = 0
    for q in case["v4_written"]:
        want = model.v4_lookup(int(ipaddress.IPv4Address(q)))
        assert _ip_answer(odb.lookup(q)) == want, q
        v4_hits += want is not None
    assert v4_hits > 100


def test_v6_only_tree_answers_ghost_ipv4(oracle):
    """tree.rs:258-277: in an IPv6-only tree the 96-zero chain ends after the two leading zero bits of 2001:db8::/32, and IPv4
    bits are read from there"""
    entries = [("2001:db8::/32", {"net": "doc"})]
    odb = oracle.Database(_build(entries))
    assert odb.metadata()["ip_version"] == 6
    model = C.TrieModel(entries)
    assert model.v4_chain_depth() == 2
    assert model.ghost_v4() == [(int(ipaddress.IPv4Address("128.4.54.224")), int(ipaddress.IPv4Address("128.4.54.227")))]
    for q, want in [("128.4.54.223", None), ("128.4.54.224", (30, {"net": "doc"})), ("128.4.54.225", (30, {"net": "doc"})),
                    ("128.4.54.226", (30, {"net": "doc"})), ("128.4.54.227", (30, {"net": "doc"})), ("128.4.54.228", None),
                    ("32.1.13.184", None), ("0.0.0.0", None)]:
        assert model.v4_in_v6only(int(ipaddress.IPv4Address(q))) == want, q
        assert _ip_answer(odb.lookup(q)) == want, q
    assert _ip_answer(odb.lookup("2001:db8::1")) == (32, {"net": "doc"}) == model.lookup(int(ipaddress.IPv6Address("2001:db8::1")))


def test_v4_tree_answers_ipv6_from_its_first_32_bits(oracle):
    """tree.rs:92-125: lookup_v6 walks from the root whatever the tree's version"""
    entries = [("32.1.13.0/24", {"net": "v4"})]
    odb = oracle.Database(_build(entries))
    assert odb.metadata()["ip_version"] == 4
    model = C.TrieModelV4(entries)
    for q, want in [("2001:d00::1", (24, {"net": "v4"})), ("2001:dff:ffff::9", (24, {"net": "v4"})), ("2001:e00::1", None),
                    ("2001:cff:ffff::1", None)]:
        assert model.v6_in_v4tree(int(ipaddress.IPv6Address(q))) == want, q
        assert _ip_answer(odb.lookup(q)) == want, q
    assert _ip_answer(odb.lookup("32.1.13.77")) == (24, {"net": "v4"}) == model.lookup(int(ipaddress.IPv4Address("32.1.13.77")))
