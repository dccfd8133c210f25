"""The rules of `matchy extract`'s output as a Python model, independent of csrc/extract_render_core.h: the order of the candidates of a
batch and the text of one candidate. Shared by test_extract_render_host.py (against the header) and test_gpu_extract_render.py (against
the library)."""

FORMATS = {"json": 0, "csv": 1, "text": 2}
TYPE_NAMES = ["Domain", "Email", "IPv4", "IPv6", "MD5", "SHA1", "SHA256", "SHA384", "SHA512", "Bitcoin", "Ethereum", "Monero"]
# line_rank of cli_main.cpp: domain, IPv4, e-mail, IPv6, the five hash types, Bitcoin, Ethereum, Monero
RANK = {0: 0, 2: 1, 1: 2, 3: 3, 4: 4, 5: 4, 6: 4, 7: 4, 8: 4, 9: 5, 10: 6, 11: 7}
LINE_BITS, RANK_BITS, START_BITS = 31, 3, 30


def record(fmt, item_type, text: bytes) -> bytes:
    name = TYPE_NAMES[item_type].lower().encode()
    if fmt == "json":
        return b'{"type":"' + name + b'","value":"' + text.replace(b"\\", b"\\\\").replace(b'"', b'\\"') + b'"}\n'
    if fmt == "csv":
        return name + b',"' + text.replace(b'"', b'""') + b'"\n'
    return text + b"\n"


def key(line, rank, start):
    assert line < 1 << LINE_BITS and rank < 1 << RANK_BITS and start < 1 << START_BITS
    return (line << (RANK_BITS + START_BITS)) | (rank << START_BITS) | start


def ordered(data: bytes, cands):
    """cands: (item_type, start, end) in any order -> the same in the order of the command: (line, rank, start)"""
    triples = [(data.count(b"\n", 0, s), RANK[t], s) for t, s, _ in cands]
    assert len({(r, s) for _, r, s in triples}) == len(triples), "two candidates share (rank, start)"
    return [c for _, c in sorted(zip(triples, cands), key=lambda p: p[0])]


def block(data: bytes, cands, fmt):
    return b"".join(record(fmt, t, data[s:e]) for t, s, e in ordered(data, cands))


# ---- the log of tests/test_gpu_extract_render.py and the child process it starts (MATCHY_AMD_HOST_PIECE_BYTES is read when the library
# first needs it, so the case that sets it runs in a process of its own: `python tests/extract_render_cases.py pieces` prints the blocks
# of the three formats as JSON; the parent, which has it unset, computes the model)
def library_log():
    import distinct_cases as D
    extra = (b'quoted "a.example.com" and \\10.9.8.7\\ and "\\alice@test.com\\"\r\n'
             b"\r\n   \n\x0c feedback.example.org\x0c\r\n"
             b"mixed 2001:db8::77 d41d8cd98f00b204e9800998ecf8427e 192.0.2.1 bob@example.org www.example.org on one line\n")
    log = D.basic_log()
    half = log.index(b"\n", len(log) // 2) + 1
    return log[:half] + extra + log[half:] + b"last line without a newline 203.0.113.9"


def candidates(ex, data):
    """what extract_chunk returns for `data`, as (item_type, start, end)"""
    return [(TYPE_NAMES.index(t), s, e) for t, s, e, _ in ex.extract_from_chunk(data)]


def main(case):
    import json
    import sys
    import matchy_amd as M
    assert case == "pieces"
    data = library_log()
    ex = M.Extractor(M.EXTRACT_ALL)
    out = {}
    for fmt in FORMATS:
        text, counts = ex.extract_rendered(data, fmt)
        out[fmt] = {"text": text.hex(), "counts": counts}
    ex.close()
    json.dump(out, sys.stdout)


if __name__ == "__main__":
    import sys
    from pathlib import Path
    ROOT = Path(__file__).resolve().parent.parent
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    main(sys.argv[1])
