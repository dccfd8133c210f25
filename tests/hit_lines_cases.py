"""Logs and the numpy model shared by tests/test_gpu_hit_lines.py. Data and the model only.

The model is the block contract of include/matchy_amd.h ("Hit lines"), written from that text: with (line, line_start, line_end) of
every hit from the definitions of tests/test_gpu_line_context.py,

    line_no      = unique(line)                                 ascending
    text         = for every k: buf[line_start_k : line_end_k] + b"\\n"
    line_off[k]  = bytes of the lines in front of k; line_off[n_lines] = len(text)
    line_of[i]   = searchsorted(line_no, line_i)

The logs are blanks with a handful of indicators, built like those of the line-context tests."""
import numpy as np

from test_gpu_line_context import DOM, IP, make_log, model


def block_model(buf, starts):
    """(text bytes, line_off, line_no, line_of) for hits that start at `starts` in buf"""
    lm = model(buf, starts)
    if not len(lm):
        return b"", np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    line_no, first = np.unique(lm[:, 0], return_index=True)
    parts = [buf[lm[i, 1]:lm[i, 2]].tobytes() + b"\n" for i in first]
    line_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return b"".join(parts), line_off, line_no.astype(np.int64), np.searchsorted(line_no, lm[:, 0]).astype(np.int64)


def from_lines(lines, final_newline=True):
    text = b"\n".join(lines) + (b"\n" if final_newline else b"")
    return np.frombuffer(text, dtype=np.uint8).copy()


def logs(M):
    S, C = M.HIT_LINES_SLICE, M.HIT_LINES_SCAN_CHUNK
    out = {}
    # a hit in the unterminated last line, and one in the first line at offset 0
    out["last_line_unterminated"] = make_log(100, [(0, IP), (60, DOM)], [50])
    out["no_newline"] = make_log(333, [(0, DOM), (200, IP)])
    # 200 hits in one line: many waves mark one bit and every record stores the line's values
    out["same_line"] = make_log(200 * 24 + 50, [(30 + 24 * i, IP if i % 2 else DOM) for i in range(200)], [7, 200 * 24 + 40])
    # hit lines on both sides of the word boundaries of the bitmap and of the first workgroup boundary of the rank step; empty lines between
    edge = 32 * C
    lines = [b""] * (edge + 40)
    for k, tok in ((0, IP), (31, DOM), (32, IP), (63, IP), (64, DOM), (edge - 1, IP), (edge, DOM), (edge + 1, IP), (edge + 39, DOM)):
        lines[k] = b"x " + tok + b" y"
    out["numbered_lines"] = from_lines(lines)
    line = b"GET /x 10.1.2.3 evil.example.com ok\r\n"
    out["crlf"] = np.frombuffer(line * 50 + b"tail 10.1.2.3\r", dtype=np.uint8).copy()
    out["line_is_its_token"] = from_lines([b"x", IP, b"", DOM, b"y", IP], final_newline=False)
    # a line of 600 KiB with a hit in its middle, then a hit line of 12 bytes: the long line is spread over the waves of 150 slices
    a = 1001 + 600 * 1024
    out["long_line"] = np.concatenate([make_log(a + 1, [(10, IP), (1001 + 300 * 1024 + 3, DOM)], [1000, a]), np.frombuffer(IP + b" abc\nrest\n", dtype=np.uint8)])
    # ill-formed UTF-8 in hit lines (input_line goes through the lossy conversion), and well-formed multi-byte text
    out["bad_utf8"] = from_lines([b"caf\xc3\xa9 " + IP + b" \xff\xfe tail \xe2\x82", b"skip \xff", "naïve ".encode() + DOM + b" \xf0\x9f\x98", b"\xc3 " + IP])
    # many hit lines: more than one workgroup of the offset step, lines of every length 0..40 around a token and every residue
    many = []
    for i in range(3 * C):
        many.append(b"." * (i % 41) + b" " + (IP if i % 3 else DOM) + b" " + b"," * (i % 7) if i % 5 else b"no hit here")
    out["many_hit_lines"] = from_lines(many)
    out["slice_edges"] = from_lines([b"-" * (S - 11) + b" " + IP, b"-" * (S - 10) + b" " + IP, b"-" * (S - 9) + b" " + IP, IP, b"-" * (S - 10) + b" " + IP])
    return out


def empty_log():
    return make_log(5000, [], range(99, 5000, 100))


def sized_log(n_lines):
    """n_lines lines of 60 bytes, two of three with a hit"""
    return from_lines([(b"%06d " % i) + (IP if i % 3 == 0 else DOM if i % 3 == 1 else b"nothing") + b" " + b"p" * 30 for i in range(n_lines)])
