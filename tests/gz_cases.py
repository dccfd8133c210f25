"""Vectors shared by tests/test_inflate_core_host.py, tests/test_gz_host.py, tests/test_gpu_gz.py and tests/test_cli_gz.py. Data only.

A case is (name, gzip file as bytes, out_len handed to the scan, expected status name, expected text or None). Expected bytes and the
verdict on every mutant come from Python's zlib; hand-made streams are written token by token with the fixed Huffman code (zlib never
emits a distance above 32 506, a stored block of length 0 in the middle, or an invalid symbol).

    good_cases()     (a) zlib streams of a small nginx-style log at the settings that reach every block type, and header variants
                     (b) hand-made: distance 32 768 at lengths 3 and 258, distance == bytes produced, a match that ends at out_len,
                         an empty stored block between two others
    reject_cases()   (c) one constructed stream per rule of the decoder, with the status it must get
    mutants(gz)      (d) every single-bit flip of the DEFLATE body and trailer, and every proper prefix that keeps the header

The case file of the C++ drivers (tests/cpp/test_inflate_core.cpp, test_gz_plan.cpp): u32 n, then per case u32 len, u32 out_len, bytes."""
import struct
import zlib

STATUS = ["OK", "BAD_HEADER", "TRUNCATED", "BAD_BLOCK", "BAD_CODES", "BAD_SYMBOL", "BAD_DISTANCE", "OVERFLOW", "SIZE_MISMATCH",
          "CRC_MISMATCH", "TRAILING_DATA"]
MD5 = "9e107d9d372bb6826bd81d3542a419d6"


def blob():
    """addresses, host names and a hash that log() mentions"""
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1)
    b.add_entry("10.1.2.0/24", {"k": "net"})
    b.add_entry("192.0.2.7", {"k": "host"})
    b.add_entry("198.51.100.0/24", {"k": "doc"})
    b.add_entry("evil.example.com", {"k": "dom"})
    b.add_entry("*.bad.example.org", {"k": "glob"})
    b.add_entry(MD5, {"k": "md5"})
    out = b.build()
    b.close()
    return out


def log(n_lines, seed=1, final_newline=True):
    """nginx-style lines; about two of three carry something the database lists"""
    x = seed * 2654435761 % (1 << 32)
    out = []
    for i in range(n_lines):
        x = (x * 1103515245 + 12345) % (1 << 31)
        ip = ["10.1.2.%d" % (x % 250), "203.0.113.%d" % (x % 199), "198.51.100.%d" % (x % 77), "192.0.2.7"][x >> 8 & 3]
        host = ["evil.example.com", "www.example.net", "cdn%d.bad.example.org" % (x % 9), "static.example.net"][x >> 12 & 3]
        tail = (" md5=" + MD5) if (x >> 16) % 5 == 0 else ""
        out.append('%s - - [19/Oct/2026:10:%02d:%02d +0000] "GET /a/%d.html HTTP/1.1" %d %d "http://%s/" "curl/8.%d"%s'
                   % (ip, i // 60 % 60, i % 60, x % 1000, [200, 404, 301][x % 3], x % 50000, host, x % 7, tail))
    text = "\n".join(out) + "\n"
    return (text if final_newline else text[:-1]).encode()


# ------------------------------------------------------------------------------------------------ gzip container
def raw_deflate(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def gz_wrap(body, text, flg=0, extra=b"", name=b"", comment=b"", crc=None, isize=None):
    """a gzip file around a raw DEFLATE body; the trailer is that of `text` unless given"""
    head = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3])
    if flg & 4:
        head += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        head += name + b"\0"
    if flg & 16:
        head += comment + b"\0"
    if flg & 2:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + body + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) & 0xFFFFFFFF if isize is None else isize)


def header_len(gz):
    """bytes in front of the DEFLATE body of a well-formed file"""
    flg, pos = gz[3], 10
    if flg & 4:
        pos += 2 + struct.unpack_from("<H", gz, pos)[0]
    for bit in (8, 16):
        if flg & bit:
            pos = gz.index(b"\0", pos) + 1
    if flg & 2:
        pos += 2
    return pos


# ------------------------------------------------------------------------------------------------ fixed-Huffman token writer
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code, most significant bit first"""
        for k in range(nbits - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Fixed(Bits):
    """blocks of the fixed code and stored blocks, token by token"""

    def block(self, final, btype):
        self.put(1 if final else 0, 1)
        self.put(btype, 2)

    def sym(self, s):
        """a literal/length symbol 0..287"""
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lits(self, data):
        for b in data:
            self.sym(b)

    def dist_sym(self, d):
        self.code(d, 5)

    def match(self, length, dist):
        li = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
        self.sym(257 + li)
        self.put(length - LEN_BASE[li], LEN_EXTRA[li])
        di = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dist_sym(di)
        self.put(dist - DIST_BASE[di], DIST_EXTRA[di])

    def eob(self):
        self.sym(256)

    def stored(self, final, data, nlen=None):
        self.block(final, 0)
        self.align()
        self.put(len(data), 16)
        self.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data


def filler(n, seed=7):
    """n bytes that do not compress to nothing and hold no newline-free run of any length that matters: short lines of hex"""
    x, out = seed, bytearray()
    while len(out) < n:
        x = (x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out += b"%016x 10.1.2.%d\n" % (x, x % 200)
    return bytes(out[:n - 1]) + b"\n"


def inflate_raw(body):
    d = zlib.decompressobj(-15)
    out = d.decompress(body)
    assert d.eof, "hand-made stream does not end"
    return out


# ------------------------------------------------------------------------------------------------ (a) + (b)
def good_cases(lines=40):
    text = log(lines)
    big = log(600, seed=3)   # ~ 60 KB: many dynamic blocks at memLevel 1, and more than one stored block of level 0 below
    out = []

    def add(case, body, t, **kw):
        out.append((case, gz_wrap(body, t, **kw), len(t), "OK", t))
    add("l6_mem1", raw_deflate(big, 6, 1), big)
    add("l1_mem1", raw_deflate(big, 1, 1), big)
    add("fixed", raw_deflate(text, 6, 8, zlib.Z_FIXED), text)
    add("stored", raw_deflate(big * 2, 0), big * 2)
    add("huffman_only", raw_deflate(text, 6, 8, zlib.Z_HUFFMAN_ONLY), text)
    add("rle", raw_deflate(text + b"=" * 300 + b"\n", 6, 8, zlib.Z_RLE), text + b"=" * 300 + b"\n")
    add("a5000", raw_deflate(b"a" * 5000, 9), b"a" * 5000)
    add("empty", raw_deflate(b""), b"")
    add("one_byte", raw_deflate(b"x"), b"x")
    nonl = log(7, seed=5, final_newline=False)
    add("no_final_newline", raw_deflate(nonl), nonl)
    add("fname", raw_deflate(text), text, flg=8, name=b"access.log")
    add("fextra", raw_deflate(text), text, flg=4, extra=b"AB\x04\x00abcd")
    add("fcomment", raw_deflate(text), text, flg=16, comment=b"rotated")
    add("fhcrc", raw_deflate(text), text, flg=2)
    add("all_header_fields", raw_deflate(text), text, flg=30, extra=b"xy", name=b"n", comment=b"c")
    # (b)
    fill = filler(32768)
    for length in (3, 258):
        w = Fixed()
        w.stored(False, fill)
        w.block(True, 1); w.match(length, 32768); w.lits(b"\n"); w.eob()
        add("dist32768_len%d" % length, w.bytes(), inflate_raw(w.bytes()))
        assert out[-1][4] == fill + fill[:length] + b"\n"
    w = Fixed(); w.block(True, 1); w.lits(b"abc"); w.match(3, 3); w.lits(b"\n"); w.eob()
    add("dist_eq_produced", w.bytes(), inflate_raw(w.bytes()))
    assert out[-1][4] == b"abcabc\n"
    w = Fixed(); w.block(True, 1); w.lits(b"10.1.2.3 x\n"); w.match(11, 11); w.eob()
    add("match_ends_at_out_len", w.bytes(), inflate_raw(w.bytes()))
    assert out[-1][4] == b"10.1.2.3 x\n" * 2
    w = Fixed(); w.stored(False, b"first 192.0.2.7\n"); w.stored(False, b""); w.stored(True, b"third evil.example.com\n")
    add("empty_stored_between", w.bytes(), inflate_raw(w.bytes()))
    return out


# ------------------------------------------------------------------------------------------------ (c)
def reject_cases():
    text = log(12, seed=9)
    body = raw_deflate(text)
    good = gz_wrap(body, text)
    out = []

    def hand(name, w, status, out_len, t=b""):
        out.append((name, gz_wrap(w.bytes(), t, isize=out_len), out_len, status, None))
    w = Fixed(); w.block(True, 1); w.match(3, 1); w.eob()
    hand("dist1_at_0", w, "BAD_DISTANCE", 3)
    w = Fixed(); w.block(True, 1); w.lits(b"ab"); w.match(3, 3); w.eob()
    hand("dist_produced_plus_1", w, "BAD_DISTANCE", 5)
    for s in (286, 287):
        w = Fixed(); w.block(True, 1); w.lits(b"abc"); w.sym(s); w.dist_sym(0); w.eob()
        hand("len_sym_%d" % s, w, "BAD_SYMBOL", 8)
    for d in (30, 31):
        w = Fixed(); w.block(True, 1); w.lits(b"abc"); w.sym(257); w.dist_sym(d); w.eob()
        hand("dist_sym_%d" % d, w, "BAD_SYMBOL", 8)
    w = Fixed(); w.block(True, 3); w.put(0, 16)
    hand("block_type_3", w, "BAD_BLOCK", 4)
    w = Fixed(); w.stored(True, b"abcd\n", nlen=0x1234)
    hand("len_nlen", w, "BAD_BLOCK", 5)
    # dynamic headers: HLIT = 257, HDIST = 1, HCLEN = 4 entries in the order 16, 17, 18, 0
    def dyn(cl):
        w = Fixed(); w.block(True, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
        for v in cl:
            w.put(v, 3)
        return w
    w = dyn([1, 1, 1, 0]); w.put(0, 32)
    hand("codes_oversubscribed", w, "BAD_CODES", 4)
    w = dyn([1, 0, 0, 1]); w.code(1, 1); w.put(0, 2); w.put(0, 32)           # symbol 16 first: nothing to repeat
    hand("repeat16_first", w, "BAD_CODES", 4)
    w = dyn([0, 0, 1, 1]); w.code(1, 1); w.put(127, 7); w.code(1, 1); w.put(127, 7); w.put(0, 32)   # 138 + 138 > 258
    hand("repeat_past_end", w, "BAD_CODES", 4)
    w = dyn([0, 0, 1, 1]); w.code(1, 1); w.put(127, 7); w.code(1, 1); w.put(109, 7); w.put(0, 32)   # 258 zero lengths: no code for 256
    hand("no_end_of_block", w, "BAD_CODES", 4)
    out.append(("one_byte_more_than_out_len", good, len(text) - 1, "OVERFLOW", None))
    out.append(("one_byte_less_than_out_len", good, len(text) + 1, "SIZE_MISMATCH", None))
    out.append(("crc_changed", gz_wrap(body, text, crc=zlib.crc32(text) ^ 0x00010000), len(text), "CRC_MISMATCH", None))
    out.append(("isize_changed", gz_wrap(body, text, isize=len(text) + 1), len(text), "SIZE_MISMATCH", None))
    out.append(("two_members", good + good, len(text), "TRAILING_DATA", None))
    out.append(("garbage_byte", good + b"\0", len(text), "TRAILING_DATA", None))
    out.append(("bad_magic", b"\x1f\x8c" + good[2:], len(text), "BAD_HEADER", None))
    out.append(("cm_not_8", good[:2] + b"\x07" + good[3:], len(text), "BAD_HEADER", None))
    out.append(("reserved_flg", good[:3] + b"\x20" + good[4:], len(text), "BAD_HEADER", None))
    out.append(("fextra_past_end", good[:3] + b"\x04" + good[4:10] + b"\xff\xff" + good[10:], len(text), "BAD_HEADER", None))
    return out


# ------------------------------------------------------------------------------------------------ (d)
def zlib_verdict(gz):
    """(accepted, output, produced_before_reject): zlib.decompressobj(31) decides; accepted means it reached the end of the member and
    nothing follows it"""
    d = zlib.decompressobj(31)
    out = b""
    try:
        for i in range(0, len(gz), 16):   # in small pieces: what was produced before an error is kept
            out += d.decompress(gz[i:i + 16])
    except zlib.error:
        return False, None, len(out) > 0
    ok = d.eof and not d.unused_data
    return ok, out if ok else None, len(out) > 0


def mutant_sources(lines=40):
    """the two streams whose mutants are taken: (name, gz, text)"""
    text = log(lines)
    return [("l6_mem1", gz_wrap(raw_deflate(text, 6, 1), text), text), ("fixed", gz_wrap(raw_deflate(text, 6, 8, zlib.Z_FIXED), text), text)]


def bit_flips(gz):
    h = header_len(gz)
    for pos in range(h, len(gz)):
        for bit in range(8):
            m = bytearray(gz)
            m[pos] ^= 1 << bit
            yield bytes(m)


def prefixes(gz):
    for n in range(header_len(gz), len(gz)):
        yield gz[:n]


def mutant_pack(gz, text, muts):
    """[(file, out_len, accepted, expected text or None)]: every odd member is the pristine stream and so is the last, so that a wave that
    writes outside its member damages bytes that are compared"""
    out = []
    for m in muts:
        ok, t, _ = zlib_verdict(m)
        out.append((m, len(text), ok, t))
        out.append((gz, len(text), True, text))
    return out


def plan_status_cap(gz, out_len):
    """what csrc/gz_plan.h decides on the host: (status, capacity) — BAD_HEADER and TRUNCATED (no room for the trailer) have capacity 0"""
    bad = len(gz) < 10 or gz[:3] != b"\x1f\x8b\x08" or bool(gz[3] & 0xE0)
    hl = 0
    if not bad:
        try:
            hl = header_len(gz)
            bad = hl > len(gz)
        except (ValueError, struct.error):
            bad = True
    if bad:
        return 1, 0
    if len(gz) - hl < 8:
        return 2, 0
    return 0, out_len or struct.unpack("<I", gz[-4:])[0]


def layout(texts_and_caps):
    """the plan's layout: [(cap, text or None)] -> (starts, batch); a failed member (None) is cap + 1 newlines, an empty one nothing"""
    starts, buf = [], bytearray()
    for cap, t in texts_and_caps:
        starts.append(len(buf))
        if cap:
            buf += (t if t is not None else b"\n" * cap) + b"\n"
    return starts, bytes(buf)


def write_case_file(path, cases):
    """cases: [(gz, out_len)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for gz, out_len in cases:
            f.write(struct.pack("<II", len(gz), out_len))
            f.write(gz)
