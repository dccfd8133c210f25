"""GPU (-m gpu): k_validate_dom decides a domain anchor from bit-sliced class masks of its 32-byte context record (domain_planes.h).
Inputs built from a pattern list — every length of the run in front of the last label around the word and context edges, every label
length, every violation of the label rules at the first, a middle and the last position of the run, non-ASCII bytes, upper case, each
pattern at four byte alignments — and lists of exactly 1, 63, 64 and 65 domain anchors, against the oracle (hits, candidates, lines)
through Scanner.scan and the device-resident entries, with databases that take each of the kernel's three modes, and through the
extractor with min_domain_labels 2 and 3."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

RUN_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 40]     # bytes in front of the last label, its dot included; >= 24: undecided path
LABELS = ["a", "io", "com", "info", "cloud", "museum", "website", "training"]    # 1..8 bytes
SEPS = [b" ", b"/", b"\"", b"\n", b":", b"=", b","]


def run(n, salt=0):
    """n domain bytes that end with the dot in front of the last label: letters and digits, one more dot in the middle from 5 bytes on."""
    if n == 0:
        return ""
    s = [chr(ord("a") + (salt + i) % 26) if (salt + i) % 7 else str((salt + i) % 10) for i in range(n)]
    s[-1] = "."
    if n >= 5:
        s[n // 2] = "."
    return "".join(s)


def inject(r, pos, s):
    return r[:pos] + s + r[pos + len(s):]


def patterns():
    out = []
    for n in RUN_LENGTHS:
        for k, l in enumerate(("com", "io", "museum")):
            out.append(run(n, n + k) + l)
    for l in LABELS:
        out += ["www.example." + l, "x." + l, l]
    # violations at the first, a middle and the last position of the run (14 bytes: inside the context; 23: it fills the context)
    for n in (14, 23):
        r = run(n, n)
        for pos in (0, n // 2 - 3, n - 2):
            out.append(inject(r, pos, "..") + "com")          # empty label
            out.append(inject(r, pos, "-.") + "com")          # label ending with '-'
        for pos in (0, n // 2 - 3, n - 3):
            out.append(inject(r, pos, ".-") + "com")          # label starting with '-'
        out.append(r + "-com")                                # ... the last label itself
        out.append(r + "com-")                                # '-' as last label byte
        out.append(r + "co-")
        out.append("." + r + "com")                           # leading '.'
        out.append("-" + r + "com")
        out.append(inject(r, 0, ".") + "com")
    # a non-boundary byte in front of the name (the separator in front stays a boundary: the name is what follows it)
    out += ["_under.example.com", "%41pct.example.org", "~tilde.example.net", "+plus.example.io", "\\back.example.com", "a_b.example.com"]
    # bytes >= 0x80 in run and label
    out += ["café.example.com", "über.example.de", "bücher.example.museum", "example.cöm", "www.example.éu", "xé.io"]
    # upper case
    out += ["WWW.EXAMPLE.COM", "www.example.COM", "Www.Example.Io", "MIXED.case.Museum", "evil.EXAMPLE.com"]
    return out


def build_log(names, head, repeat=1):
    """`head` at offset 0, then every name at the four alignments of its first byte, `repeat` times over with rotating separators."""
    buf = bytearray(head)
    k = 0
    for rep in range(repeat):
        for nm in names:
            raw = nm.encode() if isinstance(nm, str) else nm
            for a in range(4):
                buf += SEPS[k % len(SEPS)]
                while len(buf) % 4 != a:
                    buf += b" "
                buf += raw + SEPS[(k // 3 + rep) % len(SEPS)]
                k += 1
    buf += b"\n"
    return bytes(buf)


HEAD_SHORT = b"a.example.com "                            # a name at offset 0 of the buffer
HEAD_24 = (run(24, 3) + "com ").encode()                  # the label starts at byte 24 exactly: the run fills the context and starts the buffer
assert len(run(24, 3)) == 24


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


def literal_keys():
    keys = [run(n, n + k) + l for n in (7, 9, 16, 23, 24, 25, 40) for k, l in enumerate(("com", "io", "museum"))]
    keys += ["www.example.com", "x.io", "www.example.training", "a.example.com", run(24, 3) + "com", "evil.example.com", "h31.com", "h64.com",
             "h0.com", "café.example.com"]
    return keys


DATABASES = ["literals", "suffix-globs", "general-glob", "case-insensitive"]


@pytest.fixture(scope="module")
def blobs(M):
    out = {}
    for kind in DATABASES:
        b = M.DatabaseBuilder(build_epoch=11, case_insensitive=kind == "case-insensitive")
        for i, k in enumerate(literal_keys()):
            b.add_entry(k, {"k": i})
        if kind != "literals":
            for i, g in enumerate(("*.example.com", "*.example.museum", "*.io")):
                b.add_entry(g, {"g": i})
        if kind in ("general-glob", "case-insensitive"):
            b.add_entry("www.*", {"p": 1})
        out[kind] = b.build()
        b.close()
    return out


def scan_check(M, oracle, blob, buf, min_hits):
    import test_gpu_parity as parity
    gh, gl, gs, wh, wl, ws = parity._scan_both(M, oracle, blob, buf)
    assert gs == ws          # lines, candidates
    assert gh == wh
    assert gl == wl
    assert len(wh) >= min_hits
    return wh


@pytest.mark.parametrize("kind", DATABASES)
@pytest.mark.parametrize("head", ["short", "24"])
def test_pattern_list(M, oracle, blobs, kind, head):
    """The pattern list (110 names x 4 alignments) behind a name at offset 0: once (9 KiB, a few hundred anchors: one workgroup) and
    twelve times over with rotating separators (110 KiB, about 5000 anchors)."""
    buf = build_log(patterns(), HEAD_SHORT if head == "short" else HEAD_24, repeat=1 if head == "short" else 12)
    assert 4096 <= len(buf) <= 512 * 1024
    hits = scan_check(M, oracle, blobs[kind], buf, 40)
    texts = {buf[h["start"]:h["end"]].decode(errors="replace") for h in hits}
    assert (HEAD_SHORT if head == "short" else HEAD_24).decode().strip() in texts     # the name at offset 0
    for n in (7, 16, 23, 24, 25, 40):                                                  # decided here (< 24) and by the general walk (>= 24)
        assert run(n, n) + "com" in texts, n
    if kind == "suffix-globs":
        db = M.Database(blobs[kind])
        assert M.lib().matchy_amd_suffix_filter(db.handle) == 1
        db.close()


@pytest.mark.parametrize("kind", ["literals", "suffix-globs", "general-glob"])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 5000])
def test_record_counts_on_the_tile_edges_of_the_list(M, oracle, blobs, kind, count):
    """Exactly `count` dotted names in text without any other dot: the list of domain anchors ends on, one short of and one past a
    64-slot tile, holds a single record, and about 5000 (several workgroups)."""
    filler = [b" lorem ipsum ", b" dolor\tsit amet ", b"\nconsectetur ", b" adipiscing elit=", b" sed do "]
    buf = bytearray(b"begin ")
    for i in range(count):
        buf += b"h%d.com" % i + filler[i % len(filler)]
    buf = bytes(buf)
    assert buf.count(b".") == count and len(buf) <= 512 * 1024
    hits = scan_check(M, oracle, blobs[kind], buf, 1 if count < 32 else 2)
    texts = {buf[h["start"]:h["end"]].decode() for h in hits}
    assert "h0.com" in texts and (count < 65 or "h64.com" in texts)


@pytest.mark.parametrize("min_labels", [2, 3])
def test_extractor_with_min_domain_labels(M, oracle, min_labels):
    """The same inputs through the extractor (every valid name is a candidate: the dense candidate list), with the default of two labels
    and with three."""
    import test_gpu_parity as parity
    ex = M.Extractor(min_domain_labels=min_labels)
    try:
        for head in (HEAD_SHORT, HEAD_24):
            buf = build_log(patterns(), head, repeat=1 if head is HEAD_24 else 2)
            got, want = parity.norm(ex.extract_from_chunk(buf)), parity.norm(oracle.extract(buf, min_labels=min_labels))
            assert got == want
            doms = {v for (t, _, _, v) in want if t == "Domain"}
            assert len(doms) >= 30
            assert ("x.io" in doms) == (min_labels == 2) and "www.example.com" in doms
    finally:
        ex.close()
