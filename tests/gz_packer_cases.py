"""The model of csrc/gz_packer.h and the inputs tests/test_gz_packer_host.py holds it against. Written from the rules of the packer,
not from its code; built with the generators of gz_cases.py and gz_files_cases.py. Data and pure functions only.

    bounds(batch_bytes, max_member, max_carry)     (batch_bytes, max_member, carry_cap, max_text)
    Input                                          one argument of the command line: a name, what lies there, and whether it shrinks
    run(inputs, batch_bytes, members, ...)         the lines the driver prints behind its "bounds" line
    scenarios()                                    [(name, [Input])] at batch_bytes = 4096, so max_member = 1024"""
import struct
from collections import namedtuple

import gz_cases as G
import gz_files_cases as F

BATCH = 4096             # the smallest --batch-bytes the command line accepts
MAX_MEMBER = BATCH // 4


def bounds(batch_bytes, max_member=None, max_carry=None):
    bb = min(batch_bytes, (1 << 31) - (1 << 20))
    mm = bb // 4 if max_member is None else min(bb // 4, max_member)
    cc = min(1 << 20, mm) if max_carry is None else min(1 << 20, mm, max_carry)
    return bb, mm, cc, bb - cc


# kind: "file", "dir" or "missing". shrinks: the file loses its last byte between the packer's stat and its read.
Input = namedtuple("Input", "name kind data shrinks", defaults=("file", b"", False))


def isize_of(piece):
    return struct.unpack("<I", piece[-4:])[0]


def piece_ok(piece, mm):
    """a member the packer takes: at most max_member compressed, a header that parses, room for the trailer, ISIZE at most max_member"""
    body = F.parse_header(piece)
    return len(piece) <= mm and body is not None and len(piece) - body >= 8 and isize_of(piece) <= mm


def eligible(inp, bb, mm, members):
    """(isize, members) of an input that goes into a pack, or None"""
    d = inp.data
    if not inp.name.lower().endswith(".gz") or inp.kind != "file" or len(d) < 18 or len(d) > (bb if members else mm):
        return None
    if inp.shrinks:          # not whole
        return None
    body = F.parse_header(d)
    if body is None or len(d) - body < 8:
        return None
    isize, n = isize_of(d), 1
    if members:
        pieces = F.pieces(d)
        total = 0
        for p in pieces:
            if not piece_ok(p, mm):
                return None
            total += isize_of(p)
            if total + 1 > bb:
                return None
        isize, n = total, len(pieces)
    if n == 1 and (len(d) > mm or isize > mm):
        return None
    return isize, n


def run(inputs, batch_bytes, members, max_member=None, max_carry=None):
    bb, mm, _, _ = bounds(batch_bytes, max_member, max_carry)
    lines, files, at, text = [], [], 0, 0

    def flush():
        nonlocal files, at, text
        if files:
            lines.append("pack " + " ".join("%d:%d:%d:%d:%d" % f for f in files))
        files, at, text = [], 0, 0
    for i, inp in enumerate(inputs):
        e = eligible(inp, bb, mm, members)
        if e is None:
            flush()
            lines.append("single %d" % i)
            continue
        isize, n = e
        if files and (text + isize + 1 > bb or (members and at + len(inp.data) > bb)):
            flush()
        files.append((i, at, len(inp.data), isize, n))
        at += len(inp.data)
        text += isize + 1
    flush()
    return lines


# ------------------------------------------------------------------------------------------------ builders
def text_of(n, seed):
    """n bytes of log"""
    t = G.log(2 + n // 60, seed=seed)
    assert len(t) >= n
    return t[:n]


def sized(text, size, level=9):
    """one member around `text` of exactly `size` compressed bytes: an FEXTRA field takes up the difference"""
    bare = len(F.member(text, level))
    pad = size - bare - 2
    assert pad >= 0, (bare, size)
    m = F.member(text, level, flg=4, extra=b"\0" * pad)
    assert len(m) == size
    return m


def vouch(isize):
    """a small member whose trailer vouches for `isize` bytes: the packer reads the trailer, it does not inflate"""
    return G.gz_wrap(G.raw_deflate(b"x"), b"x", isize=isize)


EMPTY = F.member(b"")
HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3])


def scenarios():
    mm = MAX_MEMBER
    small = [F.member(text_of(200 + 10 * k, 300 + k)) for k in range(6)]
    out = []
    # length and header
    named = G.gz_wrap(b"", b"", flg=8, name=b"abcdef")          # 17 bytes of header, 8 of trailer: 25
    assert len(named) == 25 and F.parse_header(named) == 17
    out.append(("length_and_header", [
        Input("a.gz", data=small[0]),
        Input("b17.gz", data=(HEADER + b"\0" * 8)[:17]),
        Input("b18.gz", data=HEADER + b"\0\0\0\0" + struct.pack("<I", 5)),
        Input("bad_magic.gz", data=b"\x1f\x8c" + small[1][2:]),
        Input("reserved_flg.gz", data=small[1][:3] + b"\x20" + small[1][4:]),
        Input("c.gz", data=small[2]),
        Input("trailer7.gz", data=named[:-1]),               # 24 bytes, 7 behind the header
        Input("trailer8.gz", data=named),
        Input("d.gz", data=small[3]),
    ]))
    # name and file type
    out.append(("name_and_type", [
        Input("a.gz", data=small[0]),
        Input("b.GZ", data=small[1]),
        Input("c.Gz", data=small[2]),
        Input("d.log", data=small[3]),
        Input("e.gz", data=small[4]),
        Input("x.gz", kind="dir"),
        Input("f.gz", data=small[5]),
        Input("gone.gz", kind="missing"),
        Input("g.gzip", data=small[0]),
        Input("h.gz", data=small[1]),
    ]))
    # compressed size and ISIZE at the bound and one above it
    t = text_of(300, 310)
    at_isize, over_isize = F.member(text_of(mm, 311), 9), F.member(text_of(mm + 1, 312), 9)
    assert len(at_isize) <= mm and len(over_isize) <= mm
    out.append(("member_bounds", [
        Input("size_at.gz", data=sized(t, mm)),
        Input("size_over.gz", data=sized(t, mm + 1)),
        Input("isize_at.gz", data=at_isize),
        Input("isize_over.gz", data=over_isize),
        Input("a.gz", data=small[0]),
    ]))
    # text that lands exactly on batch_bytes: four files of max_member - 1 bytes and their separators are 4096
    exact = [F.member(text_of(mm - 1, 320 + k), 9) for k in range(4)]
    assert all(len(m) <= mm for m in exact)
    out.append(("text_exactly_batch_bytes", [Input("e%d.gz" % k, data=m) for k, m in enumerate(exact)] + [Input("next.gz", data=small[0])]))
    out.append(("text_one_byte_more", [Input("e%d.gz" % k, data=m) for k, m in enumerate(exact[:3])] + [Input("one_more.gz", data=at_isize), Input("next.gz", data=small[0])]))
    # members mode
    big = F.member(text_of(mm + 1, 330), 9)
    out.append(("members", [
        Input("two.gz", data=small[0] + small[1]),
        Input("empties_150.gz", data=EMPTY * 150),           # 3000 bytes, no text
        Input("empties_100.gz", data=EMPTY * 100),           # 2000 more: past batch_bytes compressed
        Input("empties_210.gz", data=EMPTY * 210),           # alone larger than a batch
        Input("one_member_over_isize.gz", data=small[2] + big + small[3]),
        Input("one_member_over_size.gz", data=small[2] + sized(t, mm + 1) + small[3]),
        Input("sum_batch_minus_1.gz", data=vouch(mm) * 3 + vouch(mm - 1)),
        Input("a.gz", data=small[4]),
        Input("sum_batch.gz", data=vouch(mm) * 4),
        Input("single_size_over.gz", data=sized(t, mm + 1)),
        Input("single_isize_over.gz", data=over_isize),
        Input("bgzf.gz", data=F.bgzf_file(text_of(900, 331), 97)),
        Input("second_header_broken.gz", data=small[0] + small[1][:3] + b"\x20" + small[1][4:]),
        Input("b.gz", data=small[5]),
    ]))
    # a file that shrinks behind the stat, in the middle of a run
    out.append(("shrinks", [
        Input("a.gz", data=small[0]),
        Input("b.gz", data=small[1]),
        Input("c.gz", data=small[2], shrinks=True),
        Input("d.gz", data=small[3]),
        Input("two.gz", data=small[4] + small[5], shrinks=True),
        Input("e.gz", data=small[4]),
    ]))
    return out
