"""Percent- and JSON-escaped inputs: the cases and a pure-Python reference of the decoding rules (matchy_amd/csrc/unescape_core.h).
This is the oracle of the host test and of the GPU tests, and it skips no case.

The reference is a left-to-right parser: it reads an escape where it stands and steps over it. The header decides every position on
its own from an escape mask; the two share no structure.

The rules: PERCENT decodes '%' + two hex digits and nothing else. JSON decodes a backslash + one of "\\/bfnrt and \\uXXXX (a high
surrogate escape directly followed by a low one is one code point; every other surrogate escape is EF BF BD); a backslash in front of
anything else is no escape and both bytes stay. An escape whose value is LF becomes one space, a real LF stays. Modes 3 is
percent(json(x))."""
import random
import struct

PERCENT, JSON = 1, 2
FFFD = b"\xef\xbf\xbd"
HEX = b"0123456789abcdefABCDEF"
SIMPLE = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 0x08, ord("f"): 0x0C, ord("n"): 0x0A, ord("r"): 0x0D, ord("t"): 0x09}


def _hex(data, i, n):
    """the value of the n hex digits at data[i:i + n], or None"""
    d = data[i:i + n]
    if len(d) != n or any(c not in HEX for c in d):
        return None
    return int(d, 16)


class _Out:
    def __init__(self):
        self.text, self.escapes, self.replaced, self.lf = bytearray(), 0, 0, 0

    def value(self, v):
        """one decoded escape with value v (no surrogate)"""
        self.escapes += 1
        if v == 0x0A:
            self.lf += 1
            v = 0x20
        self.text += chr(v).encode("utf-8") if v >= 0x80 else bytes([v])

    def byte(self, v):
        """one decoded escape for the BYTE v (percent: no UTF-8 encoding)"""
        self.escapes += 1
        if v == 0x0A:
            self.lf += 1
            v = 0x20
        self.text.append(v)


def _percent(data, o):
    i = 0
    while i < len(data):
        j = data.find(b"%", i)       # the literal stretch in front of the next '%' in one step
        j = len(data) if j < 0 else j
        if j > i:
            o.text += data[i:j]
            i = j
            continue
        v = _hex(data, i + 1, 2) if data[i] == 0x25 else None
        if v is None:
            o.text.append(data[i])
            i += 1
        else:
            o.byte(v)
            i += 3


def _json_unit(data, i):
    """the code unit of \\uXXXX at data[i:], or None"""
    if data[i:i + 2] != b"\\u":
        return None
    return _hex(data, i + 2, 4)


def _json(data, o):
    i = 0
    while i < len(data):
        j = data.find(b"\\", i)      # the literal stretch in front of the next backslash in one step
        j = len(data) if j < 0 else j
        if j > i:
            o.text += data[i:j]
            i = j
            continue
        c = data[i]
        if i + 1 == len(data):      # a backslash as the last byte
            o.text.append(c)
            i += 1
            continue
        d = data[i + 1]
        u = _json_unit(data, i)
        if d in SIMPLE:
            o.value(SIMPLE[d])
            i += 2
        elif u is None:             # no escape: both bytes stay, and the second one opens nothing
            o.text += data[i:i + 2]
            i += 2
        elif 0xD800 <= u <= 0xDBFF:
            lo = _json_unit(data, i + 6)
            if lo is not None and 0xDC00 <= lo <= 0xDFFF:
                o.escapes += 2
                o.text += chr(0x10000 + ((u & 0x3FF) << 10) + (lo & 0x3FF)).encode("utf-8")
                i += 12
            else:
                o.escapes += 1
                o.replaced += 1
                o.text += FFFD
                i += 6
        elif 0xDC00 <= u <= 0xDFFF:  # a low one behind a high one was read with it
            o.escapes += 1
            o.replaced += 1
            o.text += FFFD
            i += 6
        else:
            o.value(u)
            i += 6


def reference(data, modes):
    """(text, escapes, replaced, lf_escapes) of the input under the rules above"""
    assert modes in (1, 2, 3)
    o = _Out()
    if modes & JSON:
        _json(data, o)
        data = bytes(o.text)
    if modes & PERCENT:
        o.text = bytearray()
        _percent(data, o)
    return bytes(o.text), o.escapes, o.replaced, o.lf


def named_cases():
    """[(name, modes, input, text)]: the text written out by hand"""
    P, J, B = PERCENT, JSON, PERCENT | JSON
    e_pair = "\U0001F600".encode("utf-8")
    return [
        ("empty percent", P, b"", b""), ("empty json", J, b"", b""), ("empty both", B, b"", b""),
        ("plain percent", P, b"evil.com 10.1.2.3\n", b"evil.com 10.1.2.3\n"),
        ("plain json", J, b"evil.com 10.1.2.3\n", b"evil.com 10.1.2.3\n"),
        # percent
        ("%41", P, b"%41", b"A"), ("%4", P, b"%4", b"%4"), ("%", P, b"%", b"%"), ("%%41", P, b"%%41", b"%A"), ("x%", P, b"x%", b"x%"),
        ("%4 then text", P, b"%4g", b"%4g"), ("%g1", P, b"%g1", b"%g1"), ("%411", P, b"%411", b"A1"), ("%4%41", P, b"%4%41", b"%4A"),
        ("hex lower", P, b"%3a%2f%e2%82%ac", b":/\xe2\x82\xac"), ("hex upper", P, b"%3A%2F%E2%82%AC", b":/\xe2\x82\xac"), ("hex mixed", P, b"%eF%Bf", b"\xef\xbf"),
        ("%25 once", P, b"%2541", b"%41"), ("%253A", P, b"%253A", b"%3A"), ("plus stays", P, b"a+b%20c", b"a+b c"), ("%00", P, b"a%00b", b"a\x00b"),
        ("%0A is a space", P, b"a%0Ab%0ac\nd", b"a b c\nd"), ("percent ends at a line end", P, b"%4\n1", b"%4\n1"),
        ("percent leaves json alone", P, b"\\n\\u0041", b"\\n\\u0041"),
        ("issue line 1", P, b"GET /r?url=https%3A%2F%2Fevil.com%2Fpath&a=2001%3Adb8%3A%3A1 HTTP/1.1", b"GET /r?url=https://evil.com/path&a=2001:db8::1 HTTP/1.1"),
        # json: the simple escapes
        ("simple", J, b'\\"\\\\\\/\\b\\f\\r\\t', b'"\\/\x08\x0c\r\t'),
        ("\\n is a space", J, b"a\\nb", b"a b"), ("\\u000a and \\u000A", J, b"a\\u000ab\\u000Ac", b"a b c"),
        ("real LF stays", J, b"a\nb", b"a\nb"),
        ("invalid \\x", J, b"\\x41", b"\\x41"), ("invalid \\a", J, b"a\\ab", b"a\\ab"), ("invalid \\U", J, b"\\U0041", b"\\U0041"), ("invalid \\N", J, b"\\N", b"\\N"),
        ("\\u 0 digits", J, b"\\u", b"\\u"), ("\\u 0 digits then text", J, b"\\ughij", b"\\ughij"), ("\\u 1 digit", J, b"\\u0", b"\\u0"),
        ("\\u 2 digits", J, b"\\u00", b"\\u00"), ("\\u 3 digits", J, b"\\u004", b"\\u004"), ("\\u 3 digits then g", J, b"\\u004g", b"\\u004g"),
        ("\\u 3 digits then \\n", J, b"\\u004\\n", b"\\u004 "), ("\\u 4 digits", J, b"\\u0041", b"A"), ("\\u 5 digits", J, b"\\u00411", b"A1"),
        ("backslash before LF", J, b"a\\\nb", b"a\\\nb"), ("backslash before LF then n", J, b"\\\nn", b"\\\nn"),
        ("backslash last", J, b"abc\\", b"abc\\"), ("escaped backslash last", J, b"abc\\\\", b"abc\\"), ("three backslashes last", J, b"abc\\\\\\", b"abc\\\\"),
        ("only a backslash", J, b"\\", b"\\"),
        ("\\\\n is backslash n", J, b"\\\\n", b"\\n"), ("\\\\\\n is backslash space", J, b"\\\\\\n", b"\\ "), ("\\\\\\\\n", J, b"\\\\\\\\n", b"\\\\n"),
        ("escaped backslash before u", J, b"\\\\u0041", b"\\u0041"), ("three before u", J, b"\\\\\\u0041", b"\\A"),
        ("invalid escape hides the next", J, b"\\x\\n", b"\\x "), ("invalid then backslash", J, b"\\a\\\\", b"\\a\\"),
        ("\\u0000", J, b"a\\u0000b", b"a\x00b"), ("\\u007f \\u0080 \\u07ff \\u0800 \\uffff", J, b"\\u007f\\u0080\\u07ff\\u0800\\uffff", b"\x7f\xc2\x80\xdf\xbf\xe0\xa0\x80\xef\xbf\xbf"),
        ("hex cases", J, b"\\u20ac\\u20AC\\u00e9\\u00E9", b"\xe2\x82\xac\xe2\x82\xac\xc3\xa9\xc3\xa9"),
        # json: surrogates
        ("pair", J, b"\\ud83d\\ude00", e_pair), ("pair upper", J, b"\\uD83D\\uDE00", e_pair), ("pair max", J, b"\\udbff\\udfff", b"\xf4\x8f\xbf\xbf"),
        ("lone high", J, b"\\ud800", FFFD), ("lone low", J, b"\\udc00", FFFD), ("lone high then text", J, b"\\ud800abcdef", FFFD + b"abcdef"),
        ("high high low", J, b"\\ud800\\ud83d\\ude00", FFFD + e_pair), ("low low", J, b"\\udc00\\udfff", FFFD * 2), ("low high", J, b"\\udc00\\ud800", FFFD * 2),
        ("high + simple escape", J, b"\\ud83d\\n", FFFD + b" "), ("high + \\u0041", J, b"\\ud83d\\u0041", FFFD + b"A"), ("high + short \\u", J, b"\\ud83d\\ude0", FFFD + b"\\ude0"),
        ("high, gap, low", J, b"\\ud83d \\ude00", FFFD + b" " + FFFD), ("high + escaped backslash + low text", J, b"\\ud83d\\\\ude00", FFFD + b"\\ude00"),
        ("escaped backslash + high text + low", J, b"\\\\ud83d\\ude00", b"\\ud83d" + FFFD), ("pair pair", J, b"\\ud83d\\ude00\\ud83d\\ude00", e_pair * 2),
        ("pair across LF", J, b"\\ud83d\n\\ude00", FFFD + b"\n" + FFFD),
        ("json leaves percent alone", J, b"%41\\u0025", b"%41%"),
        ("issue line 2", J, b'{"msg":"{\\"host\\":\\"evil.com\\",\\"ip\\":\\"10.1.2.3\\"}"}', b'{"msg":"{"host":"evil.com","ip":"10.1.2.3"}"}'),
        ("issue line 3", J, b'{"msg":"line1\\nevil.com\\tnext","u":"https:\\/\\/evil.com\\/x","e":"evil\\u002ecom"}',
         b'{"msg":"line1 evil.com\tnext","u":"https://evil.com/x","e":"evil.com"}'),
        # both
        ("\\u002541 in both", B, b"\\u002541", b"A"), ("%5Cn in both", B, b"%5Cn", b"\\n"), ("%5cu0041 in both", B, b"%5cu0041", b"\\u0041"),
        ("\\n%0A in both", B, b"a\\nb%0Ac\nd", b"a b c\nd"), ("\\u0025\\u0034\\u0031", B, b"\\u0025\\u0034\\u0031", b"A"), ("both plain", B, b"x\\/y%2Fz", b"x/y/z"),
    ]


PERCENT_TOKENS = [b"a", b"z", b"0", b"4", b"f", b"F", b"g", b".", b"+", b" ", b"\n", b"%", b"%%", b"%4", b"%g", b"%41", b"%2e", b"%2E", b"%0a", b"%0A", b"%25", b"%00", b"%ff",
                  b"%e2%82%ac", b"\xc3\xa9", b"\\", b"%5C"]
# tokens of a valid JSON string body whose value holds neither LF nor a lone surrogate
JSON_CLEAN = [b"a", b"u", b"n", b"0", b"d", b"8", b"e", b".", b" ", b"/", b"%", b"\xc3\xa9", b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\r", b"\\t", b"\\u0041", b"\\u00e9", b"\\u00E9",
              b"\\u20ac", b"\\u0000", b"\\u005c", b"\\uffff", b"\\ud83d\\ude00", b"\\uD800\\uDC00", b"\\udbff\\udfff", b"\\\\\\\\"]
JSON_ROUGH = [b"\\", b"\\", b"\\n", b"\\u000a", b"\\u000A", b"\n", b"\\x", b"\\u", b"\\u0", b"\\u00", b"\\u004", b"\\ud800", b"\\udbff", b"\\udc00", b"\\udfff", b"\\ud83d", b"\\ude00", b'"', b"\t",
              b"\\U0041", b"u0041", b"ude00"]


def generated_cases(n_percent=2000, n_json=2600, seed=20261021):
    """[(modes, bytes)]: token soups of 0 to 12 tokens. 60 % of the JSON cases are made of clean tokens only; the others mix rough ones in"""
    rng = random.Random(seed)
    out = []
    for _ in range(n_percent):
        out.append((PERCENT, b"".join(rng.choice(PERCENT_TOKENS) for _ in range(rng.randint(0, 12)))))
    for _ in range(n_json):
        pool = JSON_CLEAN if rng.random() < 0.6 else JSON_CLEAN + JSON_ROUGH * 2
        out.append((JSON, b"".join(rng.choice(pool) for _ in range(rng.randint(0, 12)))))
    return out


def all_inputs():
    """[(name, modes, bytes)] of every named and generated case; the generated ones also under modes 3"""
    out = [(name, modes, data) for name, modes, data, _ in named_cases()]
    for k, (modes, data) in enumerate(generated_cases()):
        out.append((f"generated {k}", modes, data))
        if k % 4 == 0:
            out.append((f"generated {k} both", PERCENT | JSON, data))
    return out


def long_inputs(tile=1024):
    """[(name, modes, bytes)] of several tiles: token soups, so that every kind of escape falls on tile boundaries; backslash runs that
    span tiles; pairs at every phase"""
    rng = random.Random(4711)
    out = []
    for k, n in enumerate([300, 700, 1500]):
        out.append((f"long percent {k}", PERCENT, b"".join(rng.choice(PERCENT_TOKENS) for _ in range(n))))
        out.append((f"long json {k}", JSON, b"".join(rng.choice(JSON_CLEAN + JSON_ROUGH) for _ in range(n))))
        out.append((f"long both {k}", PERCENT | JSON, b"".join(rng.choice(JSON_CLEAN + JSON_ROUGH + PERCENT_TOKENS) for _ in range(n))))
    for shift in range(13):
        out.append((f"pairs shifted {shift}", JSON, b"x" * shift + b"\\ud83d\\ude00" * 200))
        out.append((f"units shifted {shift}", JSON, b"x" * shift + b"\\u20ac" * 400))
    for shift in range(4):
        out.append((f"percent shifted {shift}", PERCENT, b"x" * shift + b"%41" * 800))
    for run in (tile - 17, tile - 16, tile - 15, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 3 * tile + 7):
        for lead in (b"", b"x", b"x" * 15):
            out.append((f"run {run} after {len(lead)}", JSON, lead + b"\\" * run + b"n" + b"y" * 40))
            out.append((f"run {run} after {len(lead)}, high low", JSON, lead + b"\\" * run + b"ud83d\\ude00"))
    out.append(("backslashes only", JSON, b"\\" * (3 * tile + 1)))
    # the most a tile can give: a pair that begins on its last byte
    out.append(("pair on the last byte", JSON, b"x" * (tile - 1) + b"\\ud83d\\ude00" + b"y" * 30))
    out.append(("dense then pair on the last byte", JSON, b"\\u00e9" * 170 + b"xxx" + b"\\ud83d\\ude00" + b"y" * 30))
    return out


def write_case_file(path, inputs):
    """the cases as the host driver reads them: u32 count, then per case u32 modes, u32 len, bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(inputs)))
        for _, modes, data in inputs:
            f.write(struct.pack("<II", modes, len(data)))
            f.write(data)
