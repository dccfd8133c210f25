"""UTF-16 inputs: the cases and a pure-Python reference of the transcoding rules (matchy_amd/csrc/utf16_core.h). This is the oracle of
the host test and of the GPU tests, and it skips no case.

The rules: len // 2 code units in the given byte order; x < 0x80 one byte, x < 0x800 two; a high surrogate followed by a low one the
four bytes of the pair; every other surrogate EF BF BD (one U+FFFD per unit, Rust's String::from_utf16_lossy); every other unit three
bytes; an odd last byte one more EF BF BD behind everything else."""
import random
import struct

LE, BE = 0, 1
CODEC = {LE: "utf-16-le", BE: "utf-16-be"}
POOL = [0x0041, 0x000A, 0x000D, 0x002E, 0x007F, 0x0080, 0x07FF, 0x0800, 0xD7FF, 0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xE000, 0xFEFF, 0xFFFE, 0xFFFF]
FFFD = b"\xef\xbf\xbd"


def encode_units(units, order, odd_byte=None):
    """the bytes of `units` in byte order `order`, with one more byte behind them when odd_byte is not None"""
    raw = struct.pack(("<" if order == LE else ">") + "%dH" % len(units), *units)
    return raw + (bytes([odd_byte]) if odd_byte is not None else b"")


def units_of(data, order):
    return list(struct.unpack(("<" if order == LE else ">") + "%dH" % (len(data) // 2), data[:len(data) // 2 * 2]))


def is_high(x):
    return 0xD800 <= x <= 0xDBFF


def is_low(x):
    return 0xDC00 <= x <= 0xDFFF


def reference(data, order):
    """(UTF-8 bytes, code units, U+FFFD written) of the input under the rules above"""
    u = units_of(data, order)
    out, replaced, i = bytearray(), 0, 0
    while i < len(u):
        x = u[i]
        if is_high(x) and i + 1 < len(u) and is_low(u[i + 1]):
            out += chr(0x10000 + ((x & 0x3FF) << 10) + (u[i + 1] & 0x3FF)).encode("utf-8")
            i += 2
            continue
        if is_high(x) or is_low(x):
            out += FFFD
            replaced += 1
        else:
            out += chr(x).encode("utf-8")
        i += 1
    if len(data) & 1:
        out += FFFD
        replaced += 1
    return bytes(out), len(u), replaced


def codec(data, order):
    """what the interpreter's own codec makes of the input"""
    return data.decode(CODEC[order], "replace").encode("utf-8")


def codec_differs_by_rule(data, order):
    """the one place where CPython's codec and the rules differ on purpose: an input of odd length whose last whole unit is a high
    surrogate. CPython writes one U+FFFD for the two errors."""
    u = units_of(data, order)
    return bool(len(data) & 1) and bool(u) and is_high(u[-1])


def named_cases():
    """[(name, units, odd byte or None)]"""
    H, H2, L, L2 = 0xD800, 0xDBFF, 0xDC00, 0xDFFF
    cases = [
        ("empty", [], None),
        ("one byte", [], 0x41),
        ("ascii", [0x41], None), ("newline", [0x0A], None), ("7f", [0x7F], None),
        ("two bytes low", [0x80], None), ("two bytes high", [0x7FF], None),
        ("three bytes low", [0x800], None), ("three bytes d7ff", [0xD7FF], None), ("three bytes e000", [0xE000], None),
        ("feff", [0xFEFF], None), ("fffe", [0xFFFE], None), ("ffff", [0xFFFF], None),
        ("lone high", [H], None), ("lone high dbff", [H2], None), ("lone low", [L], None), ("lone low dfff", [L2], None),
        ("high low", [H, L], None), ("high low max", [H2, L2], None),
        ("high high low", [H, H2, L], None),
        ("low low", [L, L2], None),
        ("lone high last", [0x41, 0x42, H], None),
        ("lone low first", [L, 0x41, 0x42], None),
        ("high + odd byte", [0x41, H], 0xDC),
        ("pair + odd byte", [H, L], 0x00),
        ("low high", [L, H], None),
        ("ascii + odd byte", [0x41, 0x0A], 0x0A),
    ]
    return cases


def generated_cases(n=2000, seed=20260101):
    """[(units, odd byte or None)]: units drawn from POOL, 0 to 9 of them, 30 % of the inputs of odd length"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        units = [rng.choice(POOL) for _ in range(rng.randint(0, 9))]
        odd = rng.choice([0x00, 0x0A, 0x41, 0xD8, 0xDC, 0xFF]) if rng.random() < 0.3 else None
        out.append((units, odd))
    return out


def all_inputs():
    """[(name, order, bytes)] of every named and generated case in both byte orders"""
    out = []
    for order in (LE, BE):
        for name, units, odd in named_cases():
            out.append((f"{name} {CODEC[order]}", order, encode_units(units, order, odd)))
        for k, (units, odd) in enumerate(generated_cases()):
            out.append((f"generated {k} {CODEC[order]}", order, encode_units(units, order, odd)))
    return out


def write_case_file(path, inputs):
    """the cases as the host driver reads them: u32 count, then per case u32 order, u32 len, bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for _, order, data in inputs:
            f.write(struct.pack("<II", order, len(data)))
            f.write(data)


def log_text(n_lines, seed=7, crlf=False, indicators=None):
    """a log of n_lines lines as str: ASCII mostly, with lines that carry two-, three- and four-byte characters, and `indicators`
    (strings) spread over the lines"""
    rng = random.Random(seed)
    indicators = indicators or []
    extras = ["café", "über", "日本語", "€ 12", "\U0001F600 ok", "naïve \U00010437"]
    lines = []
    for i in range(n_lines):
        parts = [f"2026-01-{1 + i % 28:02d}T10:{i % 60:02d}:00Z host{i % 13} req={rng.randrange(1 << 30):08x}"]
        if indicators and rng.random() < 0.35:
            parts.append("src=" + rng.choice(indicators))
        if rng.random() < 0.2:
            parts.append(rng.choice(extras))
        if indicators and rng.random() < 0.1:
            parts.append("dst=" + rng.choice(indicators))
        lines.append(" ".join(parts))
    nl = "\r\n" if crlf else "\n"
    return nl.join(lines) + nl
