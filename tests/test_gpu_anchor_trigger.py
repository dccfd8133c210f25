"""GPU (-m gpu): k_anchor evaluates the boundary plane and the exact long-token chain only where a cheap trigger asks for them
(sparse mode) or all the time (dense mode), and offers IPv4 anchors on a relaxed look-back. Inputs built to put long tokens and
dotted text on the edges of rows, blocks and segments and to make a wave change modes; compared with the oracle through the
extractor entry and through Scanner.scan with the device-resident entries (forked, sliced, submitted on one stream)."""
import random
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu

BLOCK, ROW, SEG = 2048, 256, 8192
PROSE = b"the quick brown fox jumps over a lazy dog and runs off.\n"   # no run of letters and digits longer than 5 bytes

_rng = random.Random(20240611)
ALNUM = "ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz123456789"
HEX32 = ["5d41402abc4b2a76b9719d911017c592", "9e107d9d372bb6826bd81d3542a419d6"]
HEX64 = ["2c26b46b68ffc68ff99b453c1d30413413422d706483bfa0f98a5e886266e7ae", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"]
TOKENS = [t.encode() for t in HEX32 + HEX64] + [
    b"1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNa"[:26],                                 # 26 bytes
    "".join(_rng.choice(ALNUM) for _ in range(62)).encode(),                     # 62
    "".join(_rng.choice(ALNUM) for _ in range(110)).encode(),                    # 110
    "".join(_rng.choice("0123456789abcdef") for _ in range(128)).encode(),       # 128
]
DB_KEYS = HEX32 + HEX64 + ["1.2.3.4", "12.3.4.5", "120.0.0.0/8", "3.4.5.6", "9.9.9.9", "10.20.30.40"]


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


@pytest.fixture(scope="module")
def blob(M):
    b = M.DatabaseBuilder(build_epoch=8)
    for k in DB_KEYS:
        b.add_entry(k, {"k": k})
    out = b.build()
    b.close()
    return out


def prose(n):
    return bytearray((PROSE * (n // len(PROSE) + 1))[:n])


def put(buf, end, tok, before=b" ", after=b" "):
    """`tok` so that the byte behind it (the closing boundary) stands at `end`."""
    s = end - len(tok)
    assert s - 1 >= 0 and end < len(buf)
    buf[s - 1:s] = before
    buf[s:end] = tok
    buf[end:end + 1] = after


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


# closing boundary relative to the start of a block: first row of the block with the token starting in the last row of the block before
# (12, 3), the block's first byte (0), the last dword of the block before (-1 .. -4), lane 63 / lane 0 of rows inside the block
EDGE_OFFSETS = [12, 0, -1, -2, -4, 3, 3 * ROW - 1, 3 * ROW, 5 * ROW + 2, 7 * ROW - 3]


@pytest.mark.parametrize("rot", [0, 3, 5])
def test_long_tokens_on_row_block_and_segment_edges_in_sparse_text(M, oracle, blob, rot):
    """One token every seven blocks of prose, closing on the edges listed above, in blocks that are first, last and inside their segment.
    An input of this size is cut into 8 KiB segments, one per wave, so every token is met by a fresh wave in sparse mode: the boundary
    plane of the block and of the row in front of it come from the window (or, in a segment's first block, from the prologue). A wave
    never LEAVES dense mode here (four blocks per wave): that is test_dense_mode_is_left_and_entered_again_inside_a_segment."""
    n_blocks = 7 * len(EDGE_OFFSETS) + 8
    buf = prose(n_blocks * BLOCK)
    want_vals = []
    for i, d in enumerate(EDGE_OFFSETS):
        k = 3 + 7 * i                      # k % 4 walks through 3, 2, 1, 0: last / inner / first block of an 8 KiB segment
        tok = TOKENS[(i + rot) % len(TOKENS)]
        put(buf, k * BLOCK + d, tok)
        want_vals.append(tok)
    # ... and one as the last bytes of the buffer
    tail = TOKENS[rot % 4]
    buf[len(buf) - len(tail) - 1:] = b" " + tail
    want, hits = check(M, oracle, blob, buf, must_find=[t.decode() for t in TOKENS[:4] if t in want_vals or t == tail])
    assert len(hits) >= 1


def test_long_tokens_sparse_dense_sparse_dense(M, oracle, blob):
    """Two tokens in consecutive blocks (the second one found in dense mode by the wave that found the first), 40 blocks of prose, one more
    (a fresh wave: 8 KiB segments); runs of 20-25 letters and digits that start the chain but are too short, and runs of 200 and more,
    between them."""
    buf = prose(64 * BLOCK)
    put(buf, 5 * BLOCK + 700, TOKENS[0])
    put(buf, 6 * BLOCK + 90, TOKENS[2])
    put(buf, 7 * BLOCK - 2, TOKENS[5])
    put(buf, 7 * BLOCK + 1500, TOKENS[1])
    put(buf, 48 * BLOCK + 40, TOKENS[3])                    # starts in the last row of block 47, the last block of the segment before
    for i, n in enumerate((20, 21, 22, 23, 24, 25)):        # too short, each in a block of its own, every dword alignment
        put(buf, (12 + 3 * i) * BLOCK + 300 + i, ("a1B2" * 7)[:n].encode())
    put(buf, 33 * BLOCK + 100, b"z9" * 100)                 # 200
    put(buf, 36 * BLOCK + 5, b"Q7x" * 140)                  # 420: longer than a row, over a block edge
    put(buf, 52 * BLOCK + 1000, TOKENS[7], before=b"=", after=b"\n")
    put(buf, 56 * BLOCK + 4, TOKENS[6], before=b"\t", after=b",")
    check(M, oracle, blob, buf, must_find=HEX32 + HEX64)


def test_dense_tokens_then_prose(M, oracle, blob):
    """A token in every row for 24 blocks (dense mode from the first block on, over three segments), then prose, then tokens again."""
    line = lambda i: b'{"id":"' + TOKENS[i % 4] + b'","t":' + str(i).encode() + b"}\n"
    head = b"".join(line(i) for i in range(24 * BLOCK // 60))
    buf = bytearray(head) + prose(30 * BLOCK) + bytearray(b"".join(line(i) for i in range(200)))
    buf += prose((-len(buf)) % 64 + 64)
    assert 64 * 1024 <= len(buf) <= 256 * 1024
    check(M, oracle, blob, buf, must_find=HEX32 + HEX64)


REFUSED = [b"a12.3.4.5", b"x1.2.3.4", b"1.2.3.4.5.6", b"9.x.y.z", b"12.ab.3.4", b"1160.el7.x86"]
FOUND = [(b"Chrome/120.0.0.0", "120.0.0.0"), (b"10.20.30.40", "10.20.30.40")]


def test_ipv4_texts_the_relaxed_look_back_offers(M, oracle, blob):
    """Dotted text whose byte in front of the first octet is a letter (offered now, refused by the drain), quads with five and six
    parts, letters between the dots; beside them addresses that must be found. Every text slides over a block edge and over a segment
    edge byte by byte; an address stands at offset 0 and another one ends the buffer."""
    texts = [(t, None) for t in REFUSED] + FOUND
    buf = prose(104 * BLOCK)
    k = 2
    for t, _ in texts:
        for shift in range(0, len(t) + 1):   # one block edge per text and shift; every fourth one is a segment edge
            s = k * BLOCK - shift
            buf[s - 1:s + len(t) + 1] = b" " + t + b" "
            k += 1
    assert (k + 2) * BLOCK <= len(buf)
    buf[0:8] = b"3.4.5.6 "
    buf[len(buf) - 8:] = b" 9.9.9.9"
    want, hits = check(M, oracle, blob, buf, must_find=["120.0.0.0", "10.20.30.40", "3.4.5.6", "9.9.9.9"])
    vals = {v for (t, _, _, v) in want if t == "IPv4"}
    for v in ("12.3.4.5", "1.2.3.4", "2.3.4.5"):
        assert v not in vals, v
    assert {h["type"] for h in hits} >= {"IPv4"}


def test_dense_mode_is_left_and_entered_again_inside_a_segment(M, oracle, blob):
    """sparse -> dense -> sparse -> dense inside ONE wave. A segment is the batch divided by the resident waves (4096 on this chip), rounded
    up to 8 KiB: only a batch above 32 MiB gives a wave more than four blocks, so this input is 40 MiB (16 KiB segments; any larger multiple
    of 8 KiB works as well, the pattern below repeats every 16 KiB). Per 16 KiB: a token in block 0 (the wave enters dense mode), blocks 1-4
    prose (after the fourth quiet block it goes back to sparse mode), a token that starts in the last row of block 5 and closes in block 6
    (trigger, exact chain, boundary plane of the block AND of the previous block's last row from the window: the state a wave has after
    leaving dense mode), a too-short run in block 7. The closing edges and the tokens rotate from unit to unit."""
    unit, n_units = 8 * BLOCK, 40 * 1024 * 1024 // (8 * BLOCK)
    buf = prose(n_units * unit)
    offs = [12, 3, 0, 40, ROW + 1, 2 * ROW - 2]
    for u in range(n_units):
        base = u * unit
        put(buf, base + 900 + 4 * (u % 5) + u % 3, TOKENS[u % 4])
        put(buf, base + 6 * BLOCK + offs[u % len(offs)], TOKENS[(u + 1) % len(TOKENS)])
        put(buf, base + 7 * BLOCK + 500 + u % 4, ("a1B2" * 7)[:21 + u % 5].encode())
    check(M, oracle, blob, buf, must_find=HEX32 + HEX64)
