"""Inputs and the model shared by tests/test_whole_lines_host.py, tests/test_gpu_whole_lines.py and tests/test_cli_whole_lines.py.

Whole-line mode treats a buffer as a list of queries, one per line. The model of a batch is a plain Python line split by the rules of
the mode, and a single query per line through two independent answerers:
  * oracle.Database.lookup, the CPU restatement of the reference — for every line except those that hold both ':' and '.' (the
    oracle's query entry does not parse IPv6 text with an embedded dotted quad);
  * the library's host path, Database.query_json / matchy_query — for all lines.
For the embedded-IPv4 lines the expected answer is also written out by hand (EMBEDDED). Nothing of the model comes from a GPU scan."""
import ipaddress
import random
import re
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def kernel_units():
    """tile, bytes per lane and workgroup chunk of the streaming pass, read from csrc/whole_lines.h"""
    text = (ROOT / "matchy_amd" / "csrc" / "whole_lines.h").read_text()
    out = {}
    for name in ("WL_TILE", "WL_LANE_BYTES", "WL_WG_CHUNK"):
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert m, name
        out[name] = int(m.group(1))
    return out


# ------------------------------------------------------------------------------------------------ the rules, in Python
def split_lines(buf: bytes):
    """[(start, end)] of the queries: lines cut at '\\n', a final piece without '\\n' is a line, no empty line behind a final '\\n',
    exactly one trailing '\\r' dropped"""
    out, pos = [], 0
    while pos < len(buf):
        nl = buf.find(b"\n", pos)
        end = len(buf) if nl < 0 else nl
        q_end = end - 1 if end > pos and buf[end - 1:end] == b"\r" else end
        out.append((pos, q_end))
        pos = end + 1
    return out


def utf8_ok(q: bytes) -> bool:
    try:
        q.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def classify(q: bytes) -> str:
    """'ip4' | 'ip6' | 'str': Rust's IpAddr::from_str over the whole query (no zone, no prefix length, no blanks, no leading zeros)"""
    if not q or len(q) > 45 or any(c >= 0x80 or c in b"%/ \t" for c in q):
        return "str"
    s = q.decode("ascii")
    try:
        ipaddress.IPv4Address(s)
        return "ip4"
    except ValueError:
        pass
    try:
        ipaddress.IPv6Address(s)
        return "ip6"
    except ValueError:
        return "str"


TYPE_OF = {"ip4": "IPv4", "ip6": "IPv6", "str": "Domain"}

# queries with an embedded dotted quad, by hand: query -> (network, prefix length, data) or None for a miss
EMBEDDED = {
    b"::ffff:192.0.2.1": ("::ffff:192.0.2.0/120", 120, {"k": "mapped"}),
    b"::ffff:192.0.3.1": None,
    b"64:ff9b::192.0.2.33": ("64:ff9b::c000:221/128", 128, {"k": "nat64"}),
    b"64:ff9b::192.0.2.34": None,
    b"2001:db8:1::10.0.0.1": ("2001:db8:1::/48", 48, {"k": "net6"}),
}


def uses_oracle(q: bytes) -> bool:
    return not (b":" in q and b"." in q)


def same_network(cidr: str, q: bytes, prefix_len: int) -> bool:
    """`cidr` is the network of `prefix_len` bits the address `q` lies in (compared as networks: the spelling of an address is not the point)"""
    return ipaddress.ip_network(cidr) == ipaddress.ip_network((ipaddress.ip_address(q.decode()), prefix_len), strict=False)


def host_from_db(db):
    """the library's host path through Database.query_json (needs the library open, i.e. a GPU): q -> None, or dict(kind, prefix_len,
    cidr, ids=None, data)"""
    def answer(q: bytes):
        found, rows = db.query_json(q)
        if not rows:
            return None
        if classify(q) != "str":
            row = dict(rows[0])
            cidr, prefix = row.pop("cidr", None), row.pop("prefix_len", None)
            return dict(kind="ip", prefix_len=prefix, cidr=cidr, ids=None, data=[row])
        return dict(kind="pattern", prefix_len=0, cidr=None, ids=None, data=rows)
    return answer


def host_from_cli(answers: dict):
    """the library's host path through tests/cpp/host_lookup_cli.cpp (csrc/host_lookup.cpp, what answers matchy_query, built alone):
    `answers` maps a query to the program's JSON line"""
    def answer(q: bytes):
        r = answers[q]
        if r["kind"] == "ip":
            return dict(kind="ip", prefix_len=r["prefix_len"], cidr=None, ids=None, data=[r["data"]])
        if r["kind"] == "pattern":
            return dict(kind="pattern", prefix_len=0, cidr=None, ids=r["pattern_ids"], data=[d for d in r["data"] if d is not None])
        return None
    return answer


def oracle_answer(odb, q: bytes):
    """the oracle's single query: None, or dict(kind, prefix_len, ids, data)"""
    r = odb.lookup(q)
    if r["kind"] == "ip":
        return dict(kind="ip", prefix_len=r["prefix_len"], ids=[], data=[r["data"]])
    if r["kind"] == "pattern":
        return dict(kind="pattern", prefix_len=0, ids=r["pattern_ids"], data=[d for d in r["data"] if d is not None])
    return None


class Memo:
    """an oracle database that answers a repeated query from memory (the lists repeat their filler lines thousands of times)"""

    def __init__(self, odb):
        self.odb, self.seen = odb, {}

    def lookup(self, q):
        if q not in self.seen:
            self.seen[q] = self.odb.lookup(q)
        return self.seen[q]

    def close(self):
        self.odb.close()


def memoized(host):
    seen = {}

    def answer(q: bytes):
        if q not in seen:
            seen[q] = host(q)
        return seen[q]
    return answer


def valid_queries(buf: bytes):
    """the distinct queries of a buffer that are looked up"""
    return sorted({buf[s:e] for s, e in split_lines(buf) if utf8_ok(buf[s:e])})


def model(odb, host, buf: bytes):
    """records (one per found query, in line order) and the four counters of the batch. host: host_from_db / host_from_cli. A record:
    dict(line, start, end, type, kind, prefix_len, ids (None where neither answerer gives them), cidr (None unless the host path gives
    it), data). Asserts that the answerers agree wherever both apply, and the hand-written answers of the embedded-IPv4 lines."""
    recs = []
    ctr = dict(queries=0, address=0, string=0, invalid_utf8=0)
    for k, (s, e) in enumerate(split_lines(buf)):
        q = buf[s:e]
        ctr["queries"] += 1
        if not utf8_ok(q):
            ctr["invalid_utf8"] += 1
            continue
        cls = classify(q)
        ctr["address" if cls != "str" else "string"] += 1
        h = host(q)
        ids = h["ids"] if h is not None else None
        if uses_oracle(q):
            o = oracle_answer(odb, q)
            assert (o is None) == (h is None), (q, o, h)
            if o is not None:
                assert o["kind"] == h["kind"] and o["data"] == h["data"], (q, o, h)
                if o["kind"] == "ip":
                    assert o["prefix_len"] == h["prefix_len"], (q, o, h)
                elif ids is not None:
                    assert ids == o["ids"], (q, o, h)
                ids = o["ids"]
        if q in EMBEDDED:
            want = EMBEDDED[q]
            assert (want is None) == (h is None), (q, h)
            if want is not None:
                assert (h["prefix_len"], h["data"]) == (want[1], [want[2]]) and same_network(want[0], q, h["prefix_len"]), (q, h)
                if h["cidr"] is not None:
                    assert h["cidr"] == want[0], (q, h)
        if h is None:
            continue
        assert h["kind"] == ("pattern" if cls == "str" else "ip"), (q, h)
        recs.append(dict(line=k, start=s, end=e, type=TYPE_OF[cls], kind=h["kind"], prefix_len=h["prefix_len"], ids=ids, cidr=h["cidr"], data=h["data"]))
    return recs, ctr


def model_tally(recs, buf):
    return Counter((r["type"], buf[r["start"]:r["end"]]) for r in recs)


def build_blob(entries, case_insensitive=False):
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1, case_insensitive=case_insensitive)
    for key, data in entries:
        b.add_entry(key, data)
    blob = b.build()
    b.close()
    return blob


# ------------------------------------------------------------------------------------------------ every rule once
def rule_entries(wild=None):
    e = [("192.0.2.7", {"k": "host"}), ("1.2.3.4", {"k": "quad"}), ("10.1.2.0/24", {"k": "net"}), ("10.9.0.0/16", {"k": "net16"}),
         ("2001:db8:ffff::1", {"k": "host6"}), ("fe80::1", {"k": "linklocal"}), ("2001:db8:1::/48", {"k": "net6"}),
         ("::ffff:192.0.2.0/120", {"k": "mapped"}), ("64:ff9b::c000:221", {"k": "nat64"}),
         ("evil.com", {"k": "lit"}), ("example.com", {"k": "example"}), ("foo.com.", {"k": "rooted"}), ("hello wide world", {"k": "spaces"}),
         ("münchen.example", {"k": "umlaut"}), ("both.evil.org", {"k": "both-lit"}), ("1.2.3", {"k": "three"}),
         ("*.evil.org", {"k": "suffix"}), ("*evil*", {"k": "infix"}), ("b*.evil.org", {"k": "prefix-b"}),
         ("e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855", {"k": "sha256"})]
    if wild:
        e.append((wild, {"k": "wild"}))
    return e


HEX47 = b"abcd:" * 9 + b"ab"   # 47 bytes of hex digits and colons: longer than any address text
assert len(HEX47) == 47

RULE_QUERIES = [
    b"192.0.2.7", b"192.0.2.8", b"10.1.2.99", b"10.9.200.1", b"10.2.0.1", b"1.2.3.4",
    b"2001:db8:ffff::1", b"2001:db8:ffff::2", b"2001:db8:1::5", b"2001:DB8:1:0:0:0:0:5", b"2001:db8:2::5", b"fe80::1",
    b"::ffff:192.0.2.1", b"::ffff:192.0.3.1", b"64:ff9b::192.0.2.33", b"64:ff9b::192.0.2.34", b"2001:db8:1::10.0.0.1", b"64:ff9b::c000:221",
    b"evil.com", b"good.com", b"EXAMPLE.COM", b"example.com", b"foo.com.", b"foo.com", b"www.evil.org", b"xxevilxx", b"both.evil.org",
    b"hello wide world", b"hello  wide world", "münchen.example".encode(), "MÜNCHEN.example".encode(), "münchen.examples".encode(),
    b"01.2.3.4", b"1.2.3", b"1.2.3.4/32", b" 1.2.3.4", b"1.2.3.4 ", b"fe80::1%eth0", HEX47, b"abc", b"ab",
    b"e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855", b"E3B0C44298FC1C149AFBF4C8996FB92427AE41E4649B934CA495991B7852B855",
    b"", b"", b"\r", b"evil.com\r", b"evil.com\r\r", b"\tevil.com",
]


def rule_list():
    """the query list of case 1: every query on a line of its own ('\\r\\n' behind two of them), the last line unterminated"""
    out = bytearray()
    for i, q in enumerate(RULE_QUERIES):
        out += q + (b"\r\n" if i % 7 == 3 else b"\n")
    out += b"10.1.2.1"
    return bytes(out)


def repeats_list():
    """a list with repeats, for the tally and the line numbers"""
    qs = [b"192.0.2.7", b"evil.com", b"www.evil.org", b"miss.example", b"2001:db8:1::5", b"::ffff:192.0.2.1", b"", b"10.1.2.99", b"evil.com\r"]
    rng = random.Random(20261020)
    pool = [q for k, q in enumerate(qs) for _ in range(k + 1)]
    return b"".join(rng.choice(pool) + b"\n" for _ in range(400))


# ------------------------------------------------------------------------------------------------ invalid UTF-8
BAD_SEQUENCES = [b"\x80", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]


def invalid_list(bad: bytes):
    """`bad` once mid-line, once as the last bytes before '\\n', once as the last bytes of the buffer; valid neighbours that hit"""
    return b"evil.com\nwww." + bad + b"evil.org\n192.0.2.7\nwww.evil.org" + bad + b"\n\xe2\x82\xacevil\nevil.com\nxevil" + bad


# ------------------------------------------------------------------------------------------------ boundaries of the kernel's units
def boundary_lists(unit: int, boundary: int):
    """lists around byte offset `boundary` (a multiple of `unit`): name -> buffer"""
    B = boundary
    fill = b"pad.example\n"

    def upto(n, tail=b""):   # filler lines, then one line of 'x' so that the buffer has exactly n bytes in front of `tail`
        body = fill * (n // len(fill))
        rest = n - len(body)
        if rest == 0:
            return body
        return body[:-len(fill)] + b"x" * (len(fill) + rest - 1) + b"\n" if body else b"x" * (rest - 1) + b"\n"

    out = {}
    out["nl_last_before"] = upto(B - 9) + b"evil.com\n" + b"192.0.2.7\n" + fill
    out["nl_first_after"] = upto(B - 8) + b"evil.com" + b"\n192.0.2.7\n" + fill
    out["address_straddles"] = upto(B - 4) + b"10.1.2.99\n" + b"evil.com\n"
    out["address6_straddles"] = upto(B - 9) + b"::ffff:192.0.2.1\n" + b"evil.com\n"
    out["utf8_straddles"] = upto(B - 2) + "münchen.example".encode() + b"\n" + b"evil.com\n"
    out["utf8_4_straddles"] = upto(B - 6) + b"evil\xf0\x9f\x98\x80.x\n" + b"evil.com\n"
    out["bad_utf8_straddles"] = upto(B - 6) + b"evil\xf0\x9f\x98\n" + b"evil.com\n"
    out["bad_cont_after"] = upto(B - 5) + b"evil\n" + b"\x80evil\n" + b"evil.com\n"
    out["crlf_straddles"] = upto(B - 9) + b"evil.com\r\n" + b"192.0.2.7\r\n"
    out["long_line"] = upto(B - 5) + b"xevil" + b"y" * (2 * unit + 37) + b"\n" + b"192.0.2.7\n"
    return out


def expected_sizes_ok():
    u = kernel_units()
    assert u["WL_TILE"] == 64 * u["WL_LANE_BYTES"] and u["WL_WG_CHUNK"] % u["WL_TILE"] == 0
    return u


# ------------------------------------------------------------------------------------------------ cases that run in a process of their own
LONG_BYTES = 300000


def long_list():
    """one line of LONG_BYTES bytes that *needle* matches between short lines, and one of LONG_BYTES colons that nothing matches"""
    # the needle lies near the front: the reference's glob matcher gives up after 100 000 steps, and a needle further in than that
    # is "not found" there (and here, by parity) however the line is scanned
    long_hit = b"x" * 1000 + b"needle" + b"y" * (LONG_BYTES - 1006)
    return b"evil.com\n" + long_hit + b"\n192.0.2.7\n" + b":" * LONG_BYTES + b"\nwww.evil.org\n"


def long_entries():
    return rule_entries() + [("*needle*", {"k": "needle"})]


def hit_rows(r):
    return [[h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ids"], h["offs"], h["ip_data_offset"]] for h in r.hits()]


def main(name):
    """`pieces`: the rule list through Scanner.scan (MATCHY_AMD_HOST_PIECE_BYTES is read once per process: the parent sets it);
    `long`: the long-line list (a process of its own so that the parent's time limit is the guard). Prints the records as JSON."""
    import json
    import matchy_amd as M
    entries, data = (rule_entries(), rule_list()) if name == "pieces" else (long_entries(), long_list())
    db = M.Database(build_blob(entries))
    sc = M.Scanner(db)
    sc.set_whole_lines(True)
    r = sc.scan(data)
    out = {"hits": hit_rows(r), "lines": r.lines, "candidates": r.candidates, "counters": sc.whole_lines_counters()}
    r.close()
    sc.close()
    db.close()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    main(sys.argv[1])
