"""Databases and logs shared by tests/test_gpu_render.py. Data only.

The oracle of those tests is the host renderer on the same result (ndjson_text / ndjson_lines_text / ndjson_segments_text), so
nothing here models the text: the cases only have to reach every part of a record — IP and pattern results, several ids per hit,
payloads whose JSON needs escaping, hits and lines with quotes, CR LF and ill-formed UTF-8 — and every layout of a batch."""
import json
from pathlib import Path

import numpy as np

GOLD = Path(__file__).resolve().parent / "golden"

IPS = [b"10.1.2.3", b"10.9.9.9", b"192.0.2.7", b"2001:db8::1", b"2001:db8:0:0:0:0:0:2", b"::ffff:198.51.100.4", b"172.16.5.5"]
DOMS = [b"evil.example.com", b"bad.example.org", b"sub.wild.example.net", b"deep.sub.wild.example.net", b"xx.tracker.example.com", b"plain.example.io"]


def built_db(M):
    """IPs of both families, literals and globs; payloads with quotes, backslashes, control characters, nested maps, arrays,
    numbers of every kind; 9 distinct payloads"""
    b = M.DatabaseBuilder(build_epoch=1)
    b.add_entry("10.1.2.0/24", {"k": "net", "quote": "a \"b\" \\ c", "tab": "x\ty\n"})
    b.add_entry("10.0.0.0/8", {"k": "ten", "nested": {"a": {"b": [1, 2, {"c": "d"}]}, "e": {}}})
    b.add_entry("192.0.2.7", {"k": "host", "f": 1.5, "neg": -7, "big": 2 ** 40, "t": True})
    b.add_entry("2001:db8::/32", {"k": "v6", "u": "café €"})
    b.add_entry("::ffff:198.51.100.0/120", {"k": "mapped"})
    b.add_entry("evil.example.com", {"k": "dom", "list": ["a", "b\"c"]})
    b.add_entry("bad.example.org", {"k": "dom2"})
    b.add_entry("*.wild.example.net", {"k": "glob", "why": "one star"})
    b.add_entry("*.tracker.example.com", {"k": "glob2"})
    blob = b.build()
    b.close()
    return blob


def handmade(name):
    return (GOLD / name).read_bytes()


def handmade_log(version):
    """every query of the handmade database's expectations on a line of its own"""
    expect = json.loads((GOLD / "handmade_expect.json").read_text())[version]
    lines = [b"q%d %s end" % (i, q["query"].encode()) for i, q in enumerate(expect["queries"])]
    return b"\n".join(lines) + b"\n"


def mixed_log(n_lines=300):
    """a few hundred lines; a CR LF line, a line with ill-formed UTF-8, a hit text behind a quote, an empty line, an unterminated
    last line"""
    lines = []
    for i in range(n_lines):
        ip, dom = IPS[i % len(IPS)], DOMS[i % len(DOMS)]
        if i % 7 == 3:
            lines.append(b"nothing to see %d" % i)
        elif i % 7 == 5:
            lines.append(b"")
        elif i % 11 == 0:
            lines.append(b"GET /x \"" + dom + b"\" from " + ip + b" \\ tail\r")
        elif i % 13 == 0:
            lines.append(b"caf\xc3\xa9 \xff\xfe " + ip + b" \xe2\x82 " + dom + b" \xf0\x9f\x98")
        else:
            lines.append(b"%06d src=" % i + ip + b" host=" + dom + b" ok")
    lines.append(b"last line without an end " + IPS[0])
    return b"\n".join(lines)


def segmented_log():
    """(text, starts, sources, line_bases): five segments, one of them empty, sources that need escaping, bases above 2^32"""
    parts = [mixed_log(40) + b"\n", b"", b"only " + IPS[2] + b" here\n", mixed_log(25) + b"\n", b"tail " + DOMS[0] + b"\n"]
    starts, at = [], 0
    for p in parts:
        starts.append(at)
        at += len(p)
    sources = ["a.log", "empty \"quoted\"", "dir\\back.log", "tab\there", "café.log"]
    line_bases = [0, 5, (1 << 32) + 17, 1 << 40, 999]
    return b"".join(parts), starts, sources, line_bases


def as_array(text):
    return np.frombuffer(text, dtype=np.uint8).copy()
