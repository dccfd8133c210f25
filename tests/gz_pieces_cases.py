"""Vectors for pieces of one DEFLATE stream (Scanner.set_gz_pieces), shared by tests/test_gz_pieces_host.py, tests/test_gpu_gz_pieces.py
and tests/test_cli_gz_pieces.py, and the two calls that build and run the CPU driver (tests/cpp/test_gz_pieces.cpp). zlib in the
interpreter is the reference.

A case is (name, gzip file, piece_bytes, expected status name, expected text or None). Texts are seeded log lines (lines() here,
gz_cases.log), at most 1 MiB per member; piece_bytes is 512..4096, so a member has tens to hundreds of pieces.

    v1  1 MiB of log lines at levels 1, 6 and 9
    v2  the same text with flush(Z_BLOCK) every 20 000 input bytes: block ends at known places, back-references across every one
    v3  a whole stream under Z_FIXED; log text with incompressible stretches (stored blocks) between: no start can be found there
    v4  window edges: a hand-made fixed block with distances 32 768, 32 767 and 1 between two zlib streams (the second compressed against
        the first's last 32 KiB, so its references cross the seam); a 100 000-byte run of one byte; pieces of less than 32 KiB of text
    v5  false starts: a gzip level 0 wrapping of v1's level 6 file — the stored payload is full of genuine dynamic headers
    v6  preset dictionary: references in front of the member's first byte, first in piece 0 and first in a later piece
    v7  mutants(): single-bit flips and proper prefixes of a 64 KiB-text member at piece_bytes 1024"""
import random
import struct
import subprocess
import zlib
from pathlib import Path

import gz_cases as G

LINES_1M = 5500   # just under 1 MiB

WORDS = ["api", "v2", "users", "static", "img", "cart", "search", "login", "feed", "item", "admin", "assets", "css", "js", "order", "track"]
AGENTS = ["curl/8.4.0", "Mozilla/5.0 (X11; Linux x86_64) Gecko/20100101 Firefox/128.0", "Mozilla/5.0 (Macintosh) AppleWebKit/605.1.15 Safari/605.1.15",
          "python-requests/2.31.0", "Go-http-client/1.1", "Mozilla/5.0 (Windows NT 10.0; Win64; x64) Chrome/126.0 Safari/537.36"]


def lines(n, seed):
    """access-log lines with a request id and a path that do not repeat: about 5.5 : 1 at level 6, so that 1 MiB has ten or more DEFLATE
    blocks (G.log compresses 9 : 1 into four). About every second line carries something G.blob() lists."""
    r = random.Random(seed)
    out = []
    for i in range(n):
        x = r.getrandbits(32)
        ip = ["10.1.2.%d" % (x % 250), "203.0.113.%d" % (x % 199), "198.51.100.%d" % (x % 77), "172.%d.%d.%d" % (16 + x % 16, x >> 8 & 255, x >> 16 & 255)][x >> 28 & 3]
        host = ["evil.example.com", "www.example.net", "cdn%d.bad.example.org" % (x % 9), "static.example.net"][x >> 12 & 3]
        path = "/".join(r.choice(WORDS) for _ in range(1 + x % 4))
        tail = (" md5=" + G.MD5) if (x >> 16) % 7 == 0 else ""
        out.append('%s - - [19/Oct/2026:10:%02d:%02d +0000] "%s /%s/%d?id=%012x HTTP/1.1" %d %d "http://%s/%s" "%s" rt=0.%03d%s'
                   % (ip, i // 60 % 60, i % 60, ["GET", "POST", "HEAD"][x % 3], path, x % 100000, r.getrandbits(48), [200, 404, 301, 500][x >> 4 & 3], r.randrange(80000),
                      host, r.choice(WORDS), AGENTS[x >> 20 & 7 if (x >> 20 & 7) < 6 else 0], r.randrange(1000), tail))
    return ("\n".join(out) + "\n").encode()


def text_1m():
    return lines(LINES_1M, 11)


def deflate_blocks(data, every, level=6, zdict=None, final=True):
    """raw DEFLATE of `data` with a block end forced every `every` input bytes"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, *([zdict] if zdict else []))
    out = bytearray()
    for i in range(0, len(data), every):
        out += c.compress(data[i:i + every])
        if i + every < len(data):
            out += c.flush(zlib.Z_BLOCK)
    return bytes(out + c.flush(zlib.Z_FINISH if final else zlib.Z_SYNC_FLUSH))


def noise(n, seed):
    return random.Random(seed).randbytes(n)


def upper_lines(n, seed):
    """n bytes of lines over letters no log line has three in a row of: zlib finds no match between them and log text"""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(r.choice(b"ABDFIJKLMNQRSUVWXYZ") for _ in range(r.randrange(20, 90))) + b"\n"
    return bytes(out[:n - 1]) + b"\n"


def seam_case():
    """zlib stream A (sync-flushed: byte aligned), a non-final fixed block with the three distances, an empty stored block to align,
    zlib stream B compressed against the last 32 KiB of what precedes it"""
    a = G.log(600, seed=21)
    assert len(a) > 40000
    w = G.Fixed()
    w.out += deflate_blocks(a, 3000, final=False)
    w.block(False, 1); w.match(258, 32768); w.match(40, 32767); w.lits(b"\n="); w.match(200, 1); w.lits(b"\n"); w.eob()
    w.stored(False, b"")
    head = G.inflate_raw(bytes(w.out) + G.raw_deflate(b""))
    assert head.startswith(a + a[-32768:][:258]) and head.endswith(b"\n" + b"=" * 201 + b"\n")
    b = G.log(500, seed=21)   # the same lines again: B's references reach back across the seam
    body = bytes(w.out) + deflate_blocks(b, 3000, zdict=head[-32768:])
    text = G.inflate_raw(body)
    assert text == head + b
    return body, text


def dict_case(prefix):
    """a raw stream made with a preset dictionary inside a gzip wrapper: zlib refuses the file (distance too far back)"""
    lines = G.log(900, seed=31)
    zdict = lines[:32768]
    text = prefix + lines
    body = deflate_blocks(text, 4000, zdict=zdict)
    gz = G.gz_wrap(body, text)
    assert not G.zlib_verdict(gz)[0]
    return gz


def cases():
    out = []

    def add(name, body, text, piece_bytes, status="OK"):
        out.append((name, G.gz_wrap(body, text), piece_bytes, status, text if status == "OK" else None))
    t = text_1m()
    assert len(t) <= 1 << 20
    for level in (1, 6, 9):
        add("v1_l%d" % level, G.raw_deflate(t, level), t, 4096)
    add("v2_zblock", deflate_blocks(t, 20000), t, 4096)
    fx = G.log(1500, seed=12)
    add("v3_fixed", G.raw_deflate(fx, 6, 8, zlib.Z_FIXED), fx, 1024)
    mix = b"".join(G.log(150, seed=40 + k) + noise(9000, k) + b"\n" for k in range(6)) + G.log(150, seed=50)
    add("v3_stored_mix", deflate_blocks(mix, 7000), mix, 1024)
    body, text = seam_case()
    add("v4_seam", body, text, 512)
    run = G.log(300, seed=13) + b"a" * 100000 + b"\n" + G.log(300, seed=14)
    add("v4_run", deflate_blocks(run, 2500), run, 512)
    small = G.log(2000, seed=15)
    add("v4_short_pieces", deflate_blocks(small, 2000), small, 512)
    inner = out[1][1]
    add("v5_false_starts", G.raw_deflate(inner, 0), inner, 4096)
    out.append(("v6_dict_piece0", dict_case(b""), 512, "BAD_DISTANCE", None))
    out.append(("v6_dict_later", dict_case(upper_lines(9000, 3)), 512, "BAD_DISTANCE", None))
    return out


# ------------------------------------------------------------------------------------------------ v7
MUTANT_PIECE_BYTES = 1024


def mutant_source():
    text = G.log(505, seed=17)[:65536]
    return G.gz_wrap(deflate_blocks(text, 6000), text), text


def verdict(gz):
    """(accepted, text or None): zlib decides; accepted means it reached the end of the member and nothing follows it"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(gz)
    except zlib.error:
        return False, None
    ok = d.eof and not d.unused_data
    return ok, out if ok else None


def mutants():
    """every single-bit flip of body and trailer, then every proper prefix that keeps the header"""
    gz, _ = mutant_source()
    return list(G.bit_flips(gz)) + list(G.prefixes(gz))


def mutant_sample(n=256, seed=5):
    """a fixed sample for the GPU: indices into mutants()"""
    gz, _ = mutant_source()
    h = G.header_len(gz)
    total = (len(gz) - h) * 8 + (len(gz) - h)
    return sorted(random.Random(seed).sample(range(total), n))


def mutant_at(gz, i):
    h = G.header_len(gz)
    flips = (len(gz) - h) * 8
    if i < flips:
        m = bytearray(gz)
        m[h + i // 8] ^= 1 << (i % 8)
        return bytes(m)
    return gz[:h + (i - flips)]


# ------------------------------------------------------------------------------------------------ the CPU driver's output
def build_driver(tmp, flags=()):
    """tests/cpp/test_gz_pieces.cpp as a plain program (the sanitized build is test_inflate_core_host.build's)"""
    root = Path(__file__).resolve().parent.parent
    exe = Path(tmp) / "test_gz_pieces"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", str(root / "matchy_amd" / "csrc"), str(root / "tests" / "cpp" / "test_gz_pieces.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def run_driver(driver, tmp, cases, piece_bytes, tag=""):
    """cases: [(gz, out_len)] -> [(status name, text or None, pieces)]"""
    src, dst = Path(tmp) / ("cases%s.bin" % tag), Path(tmp) / ("out%s.bin" % tag)
    G.write_case_file(src, cases)
    r = subprocess.run([str(driver), str(src), str(dst), str(piece_bytes)], capture_output=True, text=True)
    assert r.returncode == 0 and "gz_pieces ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    return read_driver_out(dst.read_bytes(), len(cases))


def read_driver_out(raw, n):
    """[(status name, text or None, [piece tuples (start_bit, end_bit, member, produced, out_pos, flags)])]"""
    pos, out = 0, []
    for _ in range(n):
        status, ln = struct.unpack_from("<iI", raw, pos)
        pos += 8
        text = raw[pos:pos + ln] if status == 0 else None
        pos += ln
        (np,) = struct.unpack_from("<I", raw, pos)
        pos += 4
        pieces = [struct.unpack_from("<QQIIII", raw, pos + 32 * k) for k in range(np)]
        pos += 32 * np
        out.append((G.STATUS[status], text, pieces))
    assert pos == len(raw)
    return out


HAS_START, LIVE, HANDED = 1, 2, 4
