"""GPU (-m gpu): k_anchor's domain drain decides a label that fills its 8-byte window by those 8 bytes (the prefilter's Bloom filter
holds the first 8 bytes of the long last labels of the public-suffix list), and k_validate_dom refuses what the filter let through by
mistake with an exact table. Names with last labels of exactly 8 bytes, of 9 bytes and more (ASCII, xn--, raw UTF-8), long middle
labels with and without the first 8 bytes of a listed label, long last labels that are no suffix and long labels ended by a
non-boundary byte — each with its label window in the last bytes of a 2 KiB block, across the 8 KiB window wrap, in the last bytes
of a segment (final drain: the context is not resident) and at the very end of the buffer; compared with the oracle through the
extractor entry and through Scanner.scan with the device-resident entries, against a database that holds some of the names and one
that holds none."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

BLOCK, SEG = 2048, 8192
PROSE = b"the quick brown fox jumps over a lazy dog and runs off.\n"   # no dot with a letter behind it

SAUDI = b"\xd8\xa7\xd9\x84\xd8\xb3\xd8\xb9\xd9\x88\xd8\xaf\xd9\x8a\xd8\xa9"   # a listed last label of 16 bytes, raw UTF-8
# (text, the label whose 8-byte window is put on the edge)
ENTRIES = [
    (b"shop.training", b"training"),                          # last label of exactly 8 bytes
    (b"get.software", b"software"),
    (b"studio.photography", b"photography"),                  # 9 bytes and more
    (b"acme.international", b"international"),
    (b"bank.xn--mgbtx2b", b"xn--mgbtx2b"),
    (b"geld.verm\xc3\xb6gensberatung", b"verm\xc3\xb6gensberatung"),
    (b"riyadh." + SAUDI, SAUDI),
    (b"www.facebook.com", b"facebook"),                       # long middle label: starts like no listed label
    (b"www.microsoft.com", b"microsoft"),                     # ... like a listed one: gets a record, the general walk refuses it
    (b"www.americanexpress.com", b"americanexpress"),
    (b"host.localdomain", b"localdomain"),                    # long last label that is no suffix
    (b"db.internalzone", b"internalzone"),
    (b"node.trainings", b"trainings"),                        # ... and starts like one
    (b"studio.photography_x", b"photography"),                # long label ended by a non-boundary byte
    (b"get.software%20", b"software"),
    (b"example.com", b"com"),                                 # a short label beside them
]
NAME_KEYS = ["shop.training", "studio.photography", "acme.international", "bank.xn--mgbtx2b", "riyadh." + SAUDI.decode(), "www.facebook.com",
             "www.microsoft.com", "www.americanexpress.com", "example.com", "get.software"]
OTHER_KEYS = ["10.1.2.3", "unrelated.example.org", "*.evil-corp.net", "mail-*.example.net"]
MUST_FIND = ["shop.training", "get.software", "studio.photography", "acme.international", "bank.xn--mgbtx2b", "www.facebook.com",
             "www.microsoft.com", "www.americanexpress.com", "example.com"]


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


@pytest.fixture(scope="module")
def blobs(M):
    out = {}
    for name, keys in (("names", NAME_KEYS), ("none", OTHER_KEYS)):
        b = M.DatabaseBuilder(build_epoch=9)
        for k in keys:
            b.add_entry(k, {"k": k})
        out[name] = b.build()
        b.close()
    return out


def prose(n):
    return bytearray((PROSE * (n // len(PROSE) + 1))[:n])


def put(buf, j, text, label):
    """`text` between two spaces so that the first byte of `label` stands at j."""
    s = j - text.index(label)
    assert s - 1 >= 0 and s + len(text) < len(buf)
    buf[s - 1:s] = b" "
    buf[s:s + len(text)] = text
    buf[s + len(text):s + len(text) + 1] = b" "


def check(M, oracle, blob, buf, must_find=()):
    import test_gpu_parity as parity
    buf = bytes(buf)
    ex = M.Extractor()
    try:
        got, want = parity.norm(ex.extract_from_chunk(buf)), parity.norm(oracle.extract(buf))
    finally:
        ex.close()
    assert got == want
    found = {v for (_, _, _, v) in want}
    for v in must_find:
        assert v in found, v
    gh, gl, gs, wh, wl, ws = parity._scan_both(M, oracle, blob, buf)
    assert gs == ws          # lines, candidates
    assert gh == wh
    assert gl == wl
    return want, wh


@pytest.mark.parametrize("db", ["names", "none"])
def test_label_window_ends_in_the_last_bytes_of_a_block(M, oracle, blobs, db):
    """j + 8 lies 0, 3 and 7 bytes in front of the end of a 2 KiB block that does not end a segment: the window is resident when the
    block is, the bytes behind it are not yet."""
    places = [(e, d) for e in ENTRIES for d in (0, 3, 7)]
    n_blocks = len(places) * 4 // 3 + 8
    buf = prose(n_blocks * BLOCK)
    b = 1
    for (text, label), d in places:
        if (b + 1) % 4 == 0:
            b += 1
        put(buf, (b + 1) * BLOCK - d - 8, text, label)
        b += 1
    assert b < n_blocks and len(buf) <= 256 * 1024
    _, hits = check(M, oracle, blobs[db], buf, must_find=MUST_FIND)
    assert (len(hits) > 0) == (db == "names")


@pytest.mark.parametrize("db", ["names", "none"])
@pytest.mark.parametrize("rot", [0, 1])
def test_label_window_across_the_window_wrap(M, oracle, blobs, db, rot):
    """The label starts 1 to 8 bytes in front of a multiple of 8 KiB — the wrap of k_anchor's LDS window and, in inputs of this
    size, the end of a wave's segment: the anchor waits in the ring for bytes that never come and the final drain keeps it without
    its context (k_validate_dom passes such records on as they are)."""
    buf = prose((len(ENTRIES) + 2) * SEG)
    for i, (text, label) in enumerate(ENTRIES):
        put(buf, (i + 1) * SEG - (1, 4, 7, 2, 5, 8)[(i + 3 * rot) % 6], text, label)
    assert len(buf) <= 256 * 1024
    check(M, oracle, blobs[db], buf, must_find=MUST_FIND)


@pytest.mark.parametrize("db", ["names", "none"])
def test_label_in_the_last_bytes_of_a_segment(M, oracle, blobs, db):
    """The label ends with the segment (the byte behind it is the next wave's first) or, every other entry, its window does."""
    buf = prose((len(ENTRIES) + 2) * SEG)
    for i, (text, label) in enumerate(ENTRIES):
        end = (i + 1) * SEG
        put(buf, end - (len(label) if i % 2 == 0 else 8), text, label)
    assert len(buf) <= 256 * 1024
    check(M, oracle, blobs[db], buf, must_find=MUST_FIND)


@pytest.mark.parametrize("i", range(len(ENTRIES)))
def test_name_at_the_very_end_of_the_buffer(M, oracle, blobs, i):
    """The buffer ends with the name, and with the label itself (a long middle label then is a long last label at the end of the buffer);
    the database alternates from entry to entry."""
    text, label = ENTRIES[i]
    blob = blobs["names" if i % 2 == 0 else "none"]
    for cut in (len(text), text.index(label) + len(label), text.index(label) + 8):
        if cut > len(text):
            continue
        buf = prose(3 * SEG - 100 + i) + bytearray(b" ") + bytearray(text[:cut])
        check(M, oracle, blob, buf)
