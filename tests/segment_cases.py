"""Inputs and host models shared by tests/test_segments_host.py, tests/test_gpu_segments.py and tests/test_cli_pack_inputs.py.

A packed buffer is a list of segments (bytes) laid end to end; `starts` are their offsets. The host model of the device passes is
written from the definitions:

    segment_of(hit)      = searchsorted(starts, hit_start, side="right") - 1       the LAST segment whose start is <= the hit's start
    hits[s]              = hits with segment_of == s
    line_base[s]         = '\\n' bytes of buf[0, starts[s])
    lines[s]             = '\\n' bytes of buf[starts[s], starts[s + 1])
    lines_with_matches[s]= distinct lines (number of '\\n' in front of the hit) among the hits of s

The buffers come from the generator of the line-context tests (make_log: blanks, tokens at exact positions, newlines at exact
positions). `pack_model` is the model of csrc/input_packer.h.

Cases that need an environment variable read at scanner creation, or the trace, run in a process of their own:
`python tests/segment_cases.py <case>` prints JSON."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_gpu_line_context import DOM, IP, make_log   # noqa: E402

HIT_LINE, MISS_LINE = b"198.51.100.7\n", b"203.0.113.99\n"


def blob(ip_only=False, every_address=False):
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1)
    b.add_entry("10.1.2.0/24", {"k": "net"})
    b.add_entry("192.0.2.7", {"k": "host"})
    b.add_entry("198.51.100.0/24", {"k": "doc"})
    if every_address:
        b.add_entry("0.0.0.0/0", {"k": "all"})
    if not ip_only:
        b.add_entry("evil.example.com", {"k": "dom"})
        b.add_entry("*.bad.example.org", {"k": "glob"})
    out = b.build()
    b.close()
    return out


def pack(segments):
    """(buffer as uint8 array, starts) of segments laid end to end"""
    starts, pos = [], 0
    for s in segments:
        starts.append(pos)
        pos += len(s)
    return np.frombuffer(b"".join(segments), dtype=np.uint8).copy(), starts


def cut(buf, starts):
    """the segments of a buffer as bytes"""
    b = buf.tobytes()
    ends = list(starts[1:]) + [len(b)]
    return [b[s:e] for s, e in zip(starts, ends)]


def segment_of(starts, hit_starts):
    return (np.searchsorted(np.asarray(starts, dtype=np.int64), np.asarray(hit_starts, dtype=np.int64), side="right") - 1).astype(np.int64)


def table_model(buf, starts, hit_starts, lines):
    """[(start, len, hits, line_base, lines, lines_with_matches)] per segment; the three line figures are 0 without line context"""
    n = len(starts)
    ends = list(starts[1:]) + [len(buf)]
    nl = np.flatnonzero(buf == 10)
    seg = segment_of(starts, hit_starts)
    hit_line = np.searchsorted(nl, np.asarray(hit_starts, dtype=np.int64), "left")
    out = []
    for s in range(n):
        mine = seg == s
        base = int(np.searchsorted(nl, starts[s], "left"))
        upto = int(np.searchsorted(nl, ends[s], "left"))
        out.append((starts[s], ends[s] - starts[s], int(mine.sum()), base if lines else 0, upto - base if lines else 0,
                    len(np.unique(hit_line[mine])) if lines else 0))
    return out


# ------------------------------------------------------------------------------------------------ segment shapes
def short_lines(n):
    """n segments of one short line each, two of three with a hit: the edges of the sample table (1024 entries) and of its stride"""
    return [MISS_LINE if i % 3 == 2 else HIT_LINE for i in range(n)]


def tile_starts(T, C):
    """one buffer of C tiles and a bit with segments that start one byte in front of, at and one byte behind tile boundaries, and
    around the boundary between two workgroups of the prefix sum; hits on the first byte of such segments and all over"""
    L = C * T + 2 * T + 77
    at = sorted({T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 5 * T, C * T - 1, C * T, C * T + 1, C * T + T})
    newlines = sorted(set(p - 1 for p in at) | set(range(90, L, 97)))
    toks = [(0, IP), (40, DOM), (L - 8, IP)]
    toks += [(p, IP if i % 2 else DOM) for i, p in enumerate(at) if (p + 1) not in at and (p + 2) not in at]   # the first byte of a segment
    toks += [(p, IP if i % 3 else DOM) for i, p in enumerate(range(7001, L - 4096, 65521))]
    buf = make_log(L, toks, newlines)
    for p in at:
        assert buf[p - 1] == 10
    return buf, [0] + at


def shapes(T=1024, C=2048):
    """name -> (buffer, starts)"""
    out = {}
    one = make_log(4 * T + 7, [(5, IP), (T, IP), (2 * T + 1, DOM), (3 * T, IP), (4 * T - 4, IP)], [T - 1, 2 * T, 3 * T - 100])
    out["n1"] = (one, [0])
    out["n2"] = (one, [0, 2 * T + 1])
    for n in (1023, 1024, 1025, 2049):
        out[f"lines_{n}"] = pack(short_lines(n))
    a, b = b"x 10.1.2.3 y\nz evil.example.com\n", b"second 192.0.2.7 file\nwithout hits\n"
    out["empties"] = pack([b"", b"", a, b, b"", b"", b"", a, b, b""])
    out["one_byte"] = pack([b"\n", a, b"\n", b"\n", b, b"\n"])
    # a hit in the first byte of a segment, and one that ends at the last byte in front of its '\n'
    edge = b"10.1.2.3 mid evil.example.com\n"
    out["edge_hits"] = pack([edge, edge, b"192.0.2.7\n", b"www.bad.example.org\n", edge])
    out["tile_starts"] = tile_starts(T, C)
    out["unterminated_last"] = pack([a, b, b"tail 10.1.2.3 and evil.example.com"])
    out["unterminated_only"] = pack([b"10.1.2.3 evil.example.com"])
    # one segment that holds every hit beside 500 segments with none: every count of the record pass goes to one counter
    out["skew"] = pack([b"nothing here\n"] * 250 + [HIT_LINE * 6000] + [b"nothing there\n"] * 250)
    out["crlf"] = pack([b"GET /x 10.1.2.3 evil.example.com ok\r\n" * 5, b"a\r\n198.51.100.9\r\n", b"tail 10.1.2.3\r"])
    return out


# ------------------------------------------------------------------------------------------------ model of csrc/input_packer.h
def pack_model(files, batch_bytes):
    """files: [(bytes, kind)] in command-line order; kind "ok", "ineligible" (missing, .gz, a directory, ...: read the old way) or
    "unreadable" (a regular file that cannot be opened). Returns the calls of pack_inputs in order: ("pack", [(index, start,
    appended)], bytes), ("single", index), ("error", index). An empty file and one above batch_bytes / 4 are not eligible; a pack of
    one file goes the old way; a pack goes out when the next file (with the newline it needs) would pass batch_bytes."""
    plan, cur, buf = [], [], bytearray()

    def flush():
        nonlocal cur, buf
        if len(cur) == 1:
            plan.append(("single", cur[0][0]))
        elif cur:
            plan.append(("pack", cur, bytes(buf)))
        cur, buf = [], bytearray()
    for i, (data, kind) in enumerate(files):
        if kind == "ineligible" or len(data) == 0 or len(data) > batch_bytes // 4:
            flush()
            plan.append(("single", i))
            continue
        if kind == "unreadable":
            if cur and len(buf) + len(data) > batch_bytes:
                flush()
            plan.append(("error", i))
            continue
        add = 0 if data.endswith(b"\n") else 1
        if cur and len(buf) + len(data) + add > batch_bytes:
            flush()
        cur.append((i, len(buf), add))
        buf += data + (b"\n" if add else b"")
    flush()
    return plan


# ------------------------------------------------------------------------------------------------ child processes
def regrow_segments(n=60000, per=1500):
    """dense hits, one per line, as tests/test_gpu_overflow.py builds them: a fresh scanner's final_ list is over"""
    quads = [b"10.1.2.3\n", b"192.0.2.7\n", b"198.51.100.7\n", b"10.1.2.99\n"]
    lines = [quads[i % 4] for i in range(n)]
    return [b"".join(lines[i:i + per]) for i in range(0, n, per)]


PIECE_BYTES = 300 * 1024


def piece_cuts(buf, piece_bytes=PIECE_BYTES):
    """where Scanner::scan_host cuts a buffer (newline_cut of csrc/batch_reader.h): behind the last '\\n' of every window"""
    b, cuts, pos = buf.tobytes(), [], 0
    while len(b) - pos > piece_bytes:
        nl = b.rfind(b"\n", pos, pos + piece_bytes)
        pos = nl + 1 if nl >= 0 else (b.find(b"\n", pos + piece_bytes) + 1 or len(b))
        if pos < len(b):
            cuts.append(pos)
    return cuts


def pieces_case(M, at_cuts):
    """the tile_starts buffer with segments of ~70 000 bytes that straddle the pieces and a run of empty segments; at_cuts: runs of
    equal starts exactly where the pieces are cut (and in front of the first byte) as well"""
    buf, _ = tile_starts(M.LINE_TILE, M.LINE_SCAN_CHUNK)
    nl = np.flatnonzero(buf == 10)
    starts = [0] + [int(nl[np.searchsorted(nl, p)]) + 1 for p in range(70000, len(buf) - 5000, 70000)]
    starts = starts[:3] + [starts[3]] * 3 + starts[3:]   # a run of empty segments inside a piece
    if at_cuts:
        cuts = piece_cuts(buf)
        assert len(cuts) >= 5
        starts = sorted(starts + [0, 0] + [cuts[0]] * 3 + [cuts[1]] * 2 + [cuts[3]])
    return buf, starts


def result_json(r, with_of=True):
    return {"n_hits": r.n_hits, "starts": [h["start"] for h in r.hits()], "segment_of": r.segment_of if with_of else None,
            "table": [[s["start"], s["len"], s["hits"], s["line_base"], s["lines"], s["lines_with_matches"]] for s in r.segments]}


def main(case):
    import matchy_amd as M
    db = M.Database(blob())
    sc = M.Scanner(db)
    sc.set_line_context(True)
    if case == "regrow":
        buf, starts = pack(regrow_segments())
    else:   # "pieces" / "pieces_cut": MATCHY_AMD_HOST_PIECE_BYTES (= PIECE_BYTES) cuts the buffer into pieces
        buf, starts = pieces_case(M, case == "pieces_cut")
    sc.set_segments(starts)
    r = sc.scan(buf.tobytes())
    json.dump(result_json(r), sys.stdout)
    r.close(); sc.close(); db.close()


if __name__ == "__main__":
    main(sys.argv[1])
