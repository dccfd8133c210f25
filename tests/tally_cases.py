"""Inputs, the model and the child-process runner shared by tests/test_tally_host.py, tests/test_gpu_tally.py and tests/test_cli_tally.py.

The expected tally of a (database, log) pair is a Counter over the ORACLE's match set for the same bytes, keyed by
(item type name, log[start:end]); it is never derived from the product's records. `ordered` puts a Counter into the read-out order:
count descending, extractor order of the type, text bytewise ascending.

MATCHY_AMD_TALLY_* and MATCHY_AMD_TRACE are read when a scanner / its tally is created, so the cases that need them run in a process of
their own: `python tests/tally_cases.py <case>` prints, as JSON, the tally after every batch; what the trace says goes to stderr and is
read by the parent, which has none of the variables set and computes the model."""
import json
import random
import re
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

TYPE_ORDER = {"IPv6": 0, "IPv4": 1, "Email": 2, "Domain": 3, "MD5": 4, "SHA1": 4, "SHA256": 4, "SHA384": 4, "SHA512": 4,
              "Bitcoin": 5, "Ethereum": 6, "Monero": 7}
TYPE_ID = ["Domain", "Email", "IPv4", "IPv6", "MD5", "SHA1", "SHA256", "SHA384", "SHA512", "Bitcoin", "Ethereum", "Monero"]
WORDS = ["GET", "status=200", "ok", "from", "to", "user", "-", "req", "id=7", "took", "12ms", "cache", "miss"]
MD5 = "9e107d9d372bb6826bd81d3542a419d6"
SHA256 = "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"


def golden_addresses():
    """one accepted Bitcoin, Ethereum and Monero address each from tests/golden"""
    kat = json.loads((ROOT / "tests" / "golden" / "btc_eth_kat.json").read_text())
    btc = next(e["text"] for e in kat["b58"] if len(e["text"]) >= 30)
    eth = kat["eth"][0]["text"]
    xmr = json.loads((ROOT / "tests" / "golden" / "xmr_kat.json").read_text())["accept"][0]
    return btc, eth, xmr


def ordered(counter):
    """[(text, type, count)] of a Counter {(type, text): count} in read-out order"""
    rows = [(text, t, n) for (t, text), n in counter.items()]
    rows.sort(key=lambda r: (-r[2], TYPE_ORDER[r[1]], r[0], TYPE_ID.index(r[1])))
    return rows


def oracle_counter(oracle, blob, data):
    """Counter {(type, matched bytes): hits} and the number of hits, from the oracle's scan of `data`"""
    odb = oracle.Database(blob)
    hits, _, _ = odb.scan(data, want_json=False)
    odb.close()
    return Counter((h["type"], data[h["start"]:h["end"]]) for h in hits), len(hits)


def build_blob(entries, case_insensitive=False):
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1, case_insensitive=case_insensitive)
    for key, data in entries:
        b.add_entry(key, data)
    blob = b.build()
    b.close()
    return blob


# ------------------------------------------------------------------------------------------------ every type
def every_type_entries():
    btc, eth, xmr = golden_addresses()
    e = [("192.0.2.7", {"k": "host"}), ("198.51.100.9", {"k": "host2"}), ("10.1.2.0/24", {"k": "net"}), ("10.9.0.0/16", {"k": "net16"}),
         ("2001:db8:1::/48", {"k": "net6"}), ("2001:db8:ffff::1", {"k": "host6"}),
         ("evil.example.com", {"k": "dom"}), ("alice@test.com", {"k": "mail"}), (MD5, {"k": "md5"}), (SHA256, {"k": "sha256"}),
         (btc, {"k": "btc"}), (eth, {"k": "eth"}), (xmr, {"k": "xmr"}),
         ("*.bad.example.org", {"k": "glob"}), ("*@mail.example.net", {"k": "mailglob"}), ("cdn-*.example.net", {"k": "midglob"})]
    return e


def every_type_tokens():
    """(token, weight): what the log repeats. Tokens that differ only in letter case are in on purpose."""
    btc, eth, xmr = golden_addresses()
    return [("192.0.2.7", 9), ("198.51.100.9", 2), ("10.1.2.3", 7), ("10.1.2.200", 3), ("10.9.8.7", 3), ("10.9.77.1", 1), ("203.0.113.5", 4),
            ("10.1.2.77", 2), ("10.9.3.3", 1), ("2001:db8:1::5", 5), ("2001:DB8:1::5", 2), ("2001:db8:ffff::1", 3), ("2001:db8:2::1", 2), ("2001:db8:1::9", 1),
            ("mx.bad.example.org", 1), ("cdn-9.example.net", 1), ("dave@mail.example.net", 1),
            ("evil.example.com", 8), ("Evil.Example.com", 3), ("www.bad.example.org", 5), ("x.y.bad.example.org", 2), ("cdn-7.example.net", 2),
            ("good.example.com", 4), ("alice@test.com", 4), ("Alice@test.com", 2), ("bob@mail.example.net", 3), ("carol@test.com", 2),
            (MD5, 4), (MD5.upper(), 2), (SHA256, 3), ("a" * 32, 1), (btc, 2), (eth, 2), (xmr, 2)]


def make_log(rng, tokens, n_tokens):
    """lines of one to three weighted tokens between filler words"""
    pool = [t for t, w in tokens for _ in range(w)]
    out, left = [], n_tokens
    while left > 0:
        k = min(left, rng.randrange(1, 4))
        parts = [rng.choice(WORDS)]
        for _ in range(k):
            parts += [rng.choice(pool), rng.choice(WORDS)]
        parts += [rng.choice(WORDS) for _ in range(rng.randrange(2, 8))]
        out.append(" ".join(parts) + "\n")
        left -= k
    return "".join(out).encode()


def every_type_log(seed=20261018, n_tokens=900):
    return make_log(random.Random(seed), every_type_tokens(), n_tokens)


# ------------------------------------------------------------------------------------------------ many values, skew, growth, rescan
NET_ENTRIES = [("10.0.0.0/8", {"k": "ten"}), ("*.z.example.com", {"k": "zglob"})]


def value(i):
    """distinct value number i: two of three are addresses of 10/8, the third a name under z.example.com"""
    return "n%d.z.example.com" % i if i % 3 == 2 else "10.%d.%d.%d" % (1 + (i >> 16), (i >> 8) & 255, i & 255)


def values_log(rng, first, n_new, n_old):
    """one batch: values [first, first + n_new) once each and n_old draws from the values in front of them, shuffled, one per line"""
    toks = [value(i) for i in range(first, first + n_new)] + [value(rng.randrange(first)) for _ in range(n_old if first else 0)]
    rng.shuffle(toks)
    return "".join("%s %s %s\n" % (rng.choice(WORDS), t, rng.choice(WORDS)) for t in toks).encode()


def growth_batches():
    """five batches of new values, each about twice as large as the one before, with repeats of the earlier batches' values"""
    rng = random.Random(5)
    out, first = [], 0
    for n_new in (40, 80, 160, 320, 640):
        out.append(values_log(rng, first, n_new, n_new // 2))
        first += n_new
    return out


def collide_batch():
    rng = random.Random(11)
    return every_type_log(seed=3, n_tokens=300) + values_log(rng, 0, 150, 0) + values_log(rng, 150, 60, 200)


SKEW_HEAVY, SKEW_SINGLES, SKEW_CLUMP = 200000, 5000, 625


def skew_batch():
    """one address SKEW_HEAVY times and SKEW_SINGLES values once each, the singles in clumps of SKEW_CLUMP consecutive lines: a
    workgroup of the claim pass that walks through a clump meets several hundred distinct slots, more than its aggregator holds"""
    heavy = b"10.0.0.1\n"
    clumps = SKEW_SINGLES // SKEW_CLUMP
    gap = SKEW_HEAVY // clumps
    parts = []
    for c in range(clumps):
        parts.append(heavy * gap)
        parts.append("".join(value(3 * i) + "\n" for i in range(c * SKEW_CLUMP, (c + 1) * SKEW_CLUMP)).encode())
    parts.append(heavy * (SKEW_HEAVY - gap * clumps))
    return b"".join(parts)


RESCAN_QUADS = ["1.1.1.1", "2.2.2.2", "3.3.3.3", "4.4.4.4"]


def rescan_entries():
    return [(q + "/32", {"q": q}) for q in RESCAN_QUADS]


def rescan_batch(n=60000):
    """dense hits, as tests/test_gpu_overflow.py builds them: a fresh scanner's final_ list (5 000 records for 480 KB) is over"""
    return b"".join(RESCAN_QUADS[i % 4].encode() + b" " for i in range(n))


# name: (database entries, batches)
CASES = {
    "plain": lambda: (every_type_entries() + NET_ENTRIES, [collide_batch()]),
    "collide0": lambda: (every_type_entries() + NET_ENTRIES, [collide_batch()]),
    "collide4": lambda: (every_type_entries() + NET_ENTRIES, [collide_batch()]),
    "growth": lambda: (NET_ENTRIES, growth_batches()),
    "skew": lambda: (NET_ENTRIES, [skew_batch()]),
    "rescan": lambda: (rescan_entries(), [rescan_batch()]),
}

TRACE_TALLY = re.compile(r"\[matchy_amd\] tally: (\d+) records, (\d+) distinct \(\+(\d+)\), rehashes=(\d+) pool_regrows=(\d+) direct_adds=(\d+)")


def tally_rows(t):
    return [[text.hex(), typ, n] for text, typ, n in t]


def rows_of(counter):
    return [[text.hex(), typ, n] for text, typ, n in ordered(counter)]


def main(name):
    import matchy_amd as M
    entries, batches = CASES[name]()
    db = M.Database(build_blob(entries))
    sc = M.Scanner(db)
    sc.set_tally(True)
    steps = []
    for data in batches:
        r = sc.scan(data)
        t = sc.tally()
        steps.append({"n_hits": r.n_hits, "distinct": t.distinct, "matches": t.matches, "tally": tally_rows(t)})
        r.close()
    sc.close()
    db.close()
    json.dump({"steps": steps}, sys.stdout)


if __name__ == "__main__":
    main(sys.argv[1])
