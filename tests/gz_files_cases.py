"""Vectors and models shared by tests/test_gz_files_host.py, tests/test_gpu_gz_files.py and tests/test_cli_gz_members.py: gzip FILES of
one member or many. Data only; built with the helpers of gz_cases.py. Expected text comes from zlib through gzip.decompress, which
reads multi-member files.

    split_members(b)      the model of csrc/gz_plan.h gz_split_members, rule for rule
    layout_files(...)     the model of gz_plan_files' layout: members end to end, one separator behind every non-empty file
    good_files()          (name, file, text)
    reject_files()        (name, file, status name of the file)"""
import gzip
import struct
import zlib

import gz_cases as G

NEEDLE = b"192.0.2.7"   # gz_cases.blob() lists it


# ------------------------------------------------------------------------------------------------ the model of the split
SPLIT_MAX_STR = 256   # GZ_SPLIT_MAX_STR: bytes of FNAME and of FCOMMENT, the NUL included, in a header the split looks for


def parse_header(b, pos=0, end=None, max_str=None):
    """offset of the first DEFLATE byte of the member whose header starts at b[pos], or None (gz_parse_header over b[pos:end])"""
    end = len(b) if end is None else end
    if end - pos < 10 or b[pos:pos + 3] != b"\x1f\x8b\x08" or b[pos + 3] & 0xE0:
        return None
    flg, at = b[pos + 3], pos + 10
    if flg & 4:
        if end - at < 2:
            return None
        xlen = b[at] | b[at + 1] << 8
        at += 2
        if end - at < xlen:
            return None
        at += xlen
    for bit in (8, 16):
        if flg & bit:
            z = b.find(b"\0", at, end if max_str is None else min(end, at + max_str))
            if z < 0:
                return None
            at = z + 1
    if flg & 2:
        if end - at < 2:
            return None
        at += 2
    return at


def bgzf_bsize(b, pos):
    """BSIZE of the FEXTRA subfield B, C with SLEN 2 of the (parsed) header at b[pos], or None"""
    if not b[pos + 3] & 4:
        return None
    xlen = b[pos + 10] | b[pos + 11] << 8
    at, end = pos + 12, pos + 12 + xlen
    while end - at >= 4:
        slen = b[at + 2] | b[at + 3] << 8
        if end - at - 4 < slen:
            return None
        if b[at:at + 2] == b"BC" and slen == 2:
            return b[at + 4] | b[at + 5] << 8
        at += 4 + slen
    return None


def split_members(b):
    cuts, pos = [0], 0
    body = parse_header(b, 0)   # the file's first header: strings of any length; every later one: SPLIT_MAX_STR
    if body is None:
        return cuts
    while True:
        bsize = bgzf_bsize(b, pos)
        if bsize is not None:
            nxt = pos + bsize + 1
            nb = parse_header(b, nxt, max_str=SPLIT_MAX_STR) if nxt < len(b) else None
            if bsize + 1 < body - pos + 10 or nb is None:
                return cuts
        else:
            q = body + 10
            while True:
                q = b.find(b"\x1f\x8b\x08", q)
                if q < 0 or len(b) - q < 10:
                    return cuts
                nb = parse_header(b, q, max_str=SPLIT_MAX_STR) if not b[q + 3] & 0xE0 and b[q + 8] in (0, 2, 4) else None
                if nb is not None:
                    break
                q += 1
            nxt = q
        cuts.append(nxt)
        pos, body = nxt, nb


def pieces(b):
    cuts = split_members(b)
    return [b[a:e] for a, e in zip(cuts, cuts[1:] + [len(b)])]


def plan_files(files):
    """the model of gz_plan_files: (members [(file, status, cap, start)], first_member, starts, caps, total)"""
    members, first, starts, caps, start = [], [], [], [], 0
    for f, b in enumerate(files):
        first.append(len(members))
        starts.append(start)
        cap_sum = 0
        for p in pieces(b):
            status, cap = G.plan_status_cap(p, 0)
            members.append((f, status, cap, start + cap_sum))
            cap_sum += cap
        caps.append(cap_sum)
        start += cap_sum + 1 if cap_sum else 0
    first.append(len(members))
    return members, first, starts, caps, start


def layout_files(caps_and_texts):
    """[(capacity of the file, text or None for a failed file)] -> (starts, batch)"""
    return G.layout(caps_and_texts)


def file_cap(b):
    return sum(G.plan_status_cap(p, 0)[1] for p in pieces(b))


# ------------------------------------------------------------------------------------------------ builders
def member(text, level=6, **kw):
    return G.gz_wrap(G.raw_deflate(text, level), text, **kw)


def bgzf_member(text, level=6, bsize=None):
    body = G.raw_deflate(text, level)
    total = 18 + len(body) + 8
    extra = b"BC\x02\x00" + struct.pack("<H", total - 1 if bsize is None else bsize)
    return G.gz_wrap(body, text, flg=4, extra=extra)


BGZF_EOF = bgzf_member(b"")
assert len(BGZF_EOF) == 28


def bgzf_file(text, block, level=6, eof=True):
    """cut at arbitrary bytes (mid-line), the empty block last"""
    return b"".join(bgzf_member(text[i:i + block], level) for i in range(0, len(text), block)) + (BGZF_EOF if eof else b"")


def rand_concat(seed):
    """one of the random concatenations: 1-9 members, 0-60 lines each, levels 0-9, with and without a final newline -> (file, true cuts, text)"""
    x = (seed * 2654435761 + 12345) % (1 << 32)

    def nxt(n):
        nonlocal x
        x = (x * 1103515245 + 12345) % (1 << 31)
        return (x >> 8) % n
    out, cuts, text = b"", [], b""
    for k in range(1 + nxt(9)):
        n = nxt(61)
        t = G.log(n, seed=seed * 16 + k, final_newline=bool(nxt(2))) if n else b""
        cuts.append(len(out))
        out += member(t, nxt(10))
        text += t
    return out, cuts, text


def stored_false_cut():
    """a stored block that holds another .gz file: the rule cuts at the embedded header, the first piece is truncated and the second has
    trailing data"""
    inner = member(G.log(3, seed=41))
    return gzip.compress(b"head\n" + inner + b"\ntail\n", 0)


def header_patterns(n=1000, os_byte=0):
    """n bare 10-byte headers. The rule cuts at every second one (body + 10), so a piece is a header, the next header as a two-byte
    stream — 1f: final block of type 3 — and its last eight bytes as the trailer: ISIZE = os_byte << 24. With OS 0 every piece has
    capacity 0 and the file fits any pack; with OS 3 (Unix) 500 pieces vouch for 48 MiB each and the plan refuses the batch."""
    return bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, os_byte]) * n


def fname_patterns(nbytes=1 << 20):
    """one valid header, then header patterns with the FNAME bit and no zero byte anywhere behind them: every pattern is a candidate
    whose name never ends. No cut; the cost must stay linear in the length."""
    return bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3]) + bytes([0x1F, 0x8B, 8, 8, 1, 1, 1, 1, 2, 3]) * (nbytes // 10)


def straddle_file():
    """NEEDLE cut in the middle by a member boundary, on the third line of the file -> (file, text, line number)"""
    a = G.log(2, seed=51) + b"GET /x from 192.0"
    b = b".2.7 done\n" + G.log(2, seed=52)
    return member(a) + member(b, 9), a + b, 3


def good_files():
    out = []

    def add(name, f, text=None):
        t = gzip.decompress(f)
        assert text is None or t == text, name
        out.append((name, f, t))
    t = [G.log(1 + k % 7, seed=60 + k, final_newline=k % 3 != 0) for k in range(8)]
    add("two", member(t[0]) + member(t[1], 9), t[0] + t[1])
    add("three", member(t[2], 1) + member(t[3], 0) + member(t[4]), t[2] + t[3] + t[4])
    many = [G.log(1 + k % 3, seed=200 + k, final_newline=k % 5 != 0) for k in range(130)]
    add("m130", b"".join(member(m, 1 + k % 9) for k, m in enumerate(many)), b"".join(many))
    big = G.log(40, seed=70)
    add("bgzf", bgzf_file(big, 997), big)
    add("empties", member(b"") + member(t[5]) + member(b"") + member(t[6]) + member(b""), t[5] + t[6])
    add("only_empty", member(b"") + member(b"") + member(b""), b"")
    add("single", member(t[7]), t[7])
    add("one_byte_member", member(t[0]) + member(b"x") + member(b"\n" + t[1]), t[0] + b"x\n" + t[1])
    f, text, _ = straddle_file()
    add("straddle", f, text)
    add("later_headers", member(t[2]) + member(t[3], flg=8, name=b"b.log") + member(t[4], flg=16, comment=b"rotated") +
        member(t[5], flg=4, extra=b"AB\x02\x00xy") + member(t[6], flg=2) + member(t[7], flg=30, extra=b"xy", name=b"n", comment=b"c"), b"".join(t[2:8]))
    return out


def reject_files():
    """(name, file, status name of the FILE: that of its first member in stream order that is not OK)"""
    t = [G.log(2 + k, seed=80 + k) for k in range(5)]
    t[0] = b"first " + NEEDLE + b"\n" + t[0]
    ms = [member(x) for x in t]
    out = []
    bad_crc = G.gz_wrap(G.raw_deflate(t[2]), t[2], crc=zlib.crc32(t[2]) ^ 0x100)
    out.append(("crc_third_of_five", ms[0] + ms[1] + bad_crc + ms[3] + ms[4], "CRC_MISMATCH"))
    out.append(("isize_one_too_small", ms[0] + G.gz_wrap(G.raw_deflate(t[1]), t[1], isize=len(t[1]) - 1) + ms[2], "OVERFLOW"))
    out.append(("isize_one_too_large", ms[0] + G.gz_wrap(G.raw_deflate(t[1]), t[1], isize=len(t[1]) + 1) + ms[2], "SIZE_MISMATCH"))
    out.append(("stored_false_cut", stored_false_cut(), "TRUNCATED"))
    # The capacity of a piece is its last four bytes. Where a member keeps bytes that are not its own, they end here in the ISIZE of
    # that member's text, so that the stream ends at its capacity and the status is the trailer rule's, not OVERFLOW or SIZE_MISMATCH.
    out.append(("trailing_garbage", ms[0] + ms[1] + b"\0\0\0\0" + struct.pack("<I", len(t[1])), "TRAILING_DATA"))
    lying = bgzf_member(t[0], bsize=18 + len(G.raw_deflate(t[0])) + 8 + 6) + bgzf_member(t[0])   # points 7 bytes into the next member: no header there
    out.append(("lying_bsize", lying, "TRAILING_DATA"))
    out.append(("header_patterns", header_patterns(), "BAD_BLOCK"))
    second = bytearray(ms[0]); second[3] |= 0x20
    out.append(("reserved_flg_in_second", ms[0] + bytes(second), "TRAILING_DATA"))
    # two different failures: SIZE_MISMATCH in the second member, CRC_MISMATCH in the fourth; the first in stream order decides
    out.append(("two_failures", ms[0] + G.gz_wrap(G.raw_deflate(t[1]), t[1], isize=len(t[1]) + 1) + ms[2] + bad_crc + ms[4], "SIZE_MISMATCH"))
    return out


def zlib_accepts(b):
    try:
        return True, gzip.decompress(b)
    except Exception:
        return False, None


def mutant_source():
    """a three-member file of about 600 compressed bytes"""
    t = [G.log(3, seed=91), G.log(2, seed=92, final_newline=False), b"\n" + G.log(2, seed=93)]
    return member(t[0]) + member(t[1], 9) + member(t[2], 1), b"".join(t)


def all_bit_flips(b):
    for pos in range(len(b)):
        for bit in range(8):
            m = bytearray(b)
            m[pos] ^= 1 << bit
            yield bytes(m)
