"""IPv4, e-mail, domain and file-hash models and generators shared by test_extract_model_host.py (CPU) and
test_gpu_extract_model.py (GPU). No GPU, no project code, nothing from oracle/: the models restate the reference's chunk
path (matchy-extractor/src/lib.rs) line by line in Python, the suffix set is read from matchy_amd/data/psl.bin (data; the
container is described in tools/gen_psl.py) with a decoder of its own.

Every model function takes skip=(rule names): the named rules are switched off. The tests use that to count, per corpus, the
tokens whose verdict hangs on each rule. Rules that no input can make decide a verdict on their own are listed in UNOBSERVABLE
with the reason."""
import bisect
import ipaddress
import random
import re
import struct
from pathlib import Path

PSL_PATH = Path(__file__).resolve().parent.parent / "matchy_amd" / "data" / "psl.bin"

EX_DOMAIN, EX_EMAIL, EX_IPV4, EX_IPV6, EX_HASH = 1, 2, 4, 8, 16
FOUR = EX_DOMAIN | EX_EMAIL | EX_IPV4 | EX_HASH
HASH_TYPES = {32: "MD5", 40: "SHA1", 64: "SHA256", 96: "SHA384", 128: "SHA512"}    # HashType::from_len (lib.rs:160-170)
FOUR_TYPES = frozenset(["IPv4", "Email", "Domain"] + list(HASH_TYPES.values()))

# (flags, min_labels): all extractors, each of the four alone, the four without the rest, domains at 1 / 2 / 3 labels
SETTINGS = [(255, 2), (EX_IPV4, 2), (EX_EMAIL, 2), (EX_DOMAIN, 2), (EX_HASH, 2), (FOUR, 2), (EX_DOMAIN, 1), (EX_DOMAIN, 3), (FOUR, 1), (FOUR, 3)]


# ------------------------------------------------------------------------------------------------ classes and suffix set
_ALNUM = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789")
_LETTER = frozenset(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ")
_DIGIT = frozenset(b"0123456789")
_DIGDOT = frozenset(b"0123456789.")
_HEX = frozenset(b"0123456789abcdefABCDEF")
BOUNDARY = frozenset(b" \t\n\r/,;:()[]{}<>\"'@=")                      # BOUNDARY_LOOKUP (lib.rs:1568-1593): 20 bytes
DOMAIN_FAST = _ALNUM | frozenset(b"-.") | frozenset(range(0x80, 0x100))   # is_domain_char_fast (lib.rs:1597-1629, 1658-1660)
DOMAIN_ASCII = _ALNUM | frozenset(b"-.")                                  # is_domain_char (lib.rs:1639-1641)
EMAIL_LOCAL = _ALNUM | frozenset(b".-_+")                                 # is_email_local_char (lib.rs:1644-1647)
assert len(BOUNDARY) == 20

_TOKEN_RE = re.compile(b"[^" + re.escape(bytes(sorted(BOUNDARY))) + b"]+")
_HEXRUN_RE = re.compile(b"[0-9a-fA-F]+")


def load_psl(path=PSL_PATH):
    """the PSLB v1 container: header "PSLB", version, count, payload bytes (u32 little endian each), then front-coded entries
    (u8 shared with the previous entry, u8 rest, rest bytes) -> frozenset of byte strings"""
    blob = Path(path).read_bytes()
    magic, version, count, nbytes = struct.unpack_from("<4sIII", blob, 0)
    assert magic == b"PSLB" and version == 1 and len(blob) == 16 + nbytes
    out, prev, pos = [], b"", 16
    for _ in range(count):
        shared, rest = blob[pos], blob[pos + 1]
        prev = prev[:shared] + blob[pos + 2:pos + 2 + rest]
        pos += 2 + rest
        out.append(prev)
    assert pos == len(blob) and len(set(out)) == count
    return frozenset(out)


_PSL = None


def psl():
    global _PSL
    if _PSL is None:
        _PSL = load_psl()
    return _PSL


def find_suffix(cand):
    """find_valid_tld_suffix_bytes (lib.rs:1671-1692): from the LAST dot backwards, the first listed suffix wins -> position of
    its dot | None. The set holds the list's lines as they stand: "*.ck" is a string that no candidate can contain, "ck" is not
    listed, and the snapshot has no exception ("!") lines, so neither foo.ck nor www.ck has a suffix."""
    s = psl()
    i = cand.rfind(b".")
    while i >= 0:
        if cand[i + 1:] in s:
            return i
        i = cand.rfind(b".", 0, i)
    return None


_DIGDOT_RE = re.compile(b"[0-9.]+")
_DOMAIN_RE = re.compile(b"[0-9A-Za-z.\\x80-\\xff-]+")


def _runs(buf, regex):
    """the maximal runs of a byte class -> function: position inside a run -> (start, end) of that run (what the reference's
    byte-by-byte walks to both sides of the position arrive at)"""
    spans = [m.span() for m in regex.finditer(buf)]
    starts = [s for s, _ in spans]
    return lambda pos: spans[bisect.bisect_right(starts, pos) - 1]


def _positions(buf, needle):
    out, i = [], buf.find(needle)
    while i >= 0:
        out.append(i)
        i = buf.find(needle, i + 1)
    return out


# Rules that cannot decide a verdict alone, and why (the tests assert that switching them off changes nothing on any corpus):
UNOBSERVABLE = {
    "ipv4.edge": "dot == 0 / dot + 6 > len only keep the indexing in bounds: the shortest tail of a quad behind its first dot is 6 bytes",
    "ipv4.digit_sides": "an accepted quad has digits on both sides of all three dots, and every dot of a run leads to the same parse",
    "ipv4.dots3": "the three dots of an accepted quad lie within 11 bytes of its start, so the first dot always counts three",
    "ipv4.dots_from_i": "counting from the run's start instead of from the current dot admits more dots; the same parse decides them",
    "ipv4.max3": "four digits without a leading zero are more than 255",
    "email.local_nonempty": "an empty local part has no letter",
    "email.domain_nonempty": "an empty domain part has no dot",
    "email.domain_dot": "without a dot no suffix is found",
    "domain.content": "a dot at the start of the run makes an empty label; behind a dot at the end no suffix is listed",
    "domain.bare": "the suffix search returns a dot's position: position 0 means an empty first label",
    "domain.accept_only": "every dot of a run sees the same candidate, so a cursor moved by rejects too skips only dots that are rejected again",
}


# ------------------------------------------------------------------------------------------------ IPv4
def _parse_ipv4(buf, start, skip):
    """try_parse_ipv4 (lib.rs:813-869) -> end | None"""
    n = len(buf)
    if "boundary_front" not in skip and start > 0 and buf[start - 1] not in BOUNDARY:
        return None
    pos = start
    for k in range(4):
        first, value, digits = pos, 0, 0
        while pos < n and buf[pos] in _DIGIT and (digits < 3 or "max3" in skip):
            value = value * 10 + buf[pos] - 48
            pos += 1
            digits += 1
        if digits == 0:
            return None
        if value > 255 and "le255" not in skip:
            return None
        if digits > 1 and buf[first] == 48 and "leading_zero" not in skip:
            return None
        if k < 3:
            if pos >= n or buf[pos] != 46:
                return None
            pos += 1
    if "boundary_behind" not in skip and pos < n and buf[pos] not in BOUNDARY:
        return None
    return pos


def model_ipv4(buf, skip=()):
    """extract_ipv4_chunk_with_dots (lib.rs:1120-1179) -> [(start, end)]"""
    buf = bytes(buf)
    n = len(buf)
    dots = _positions(buf, b".")
    run_of = _runs(buf, _DIGDOT_RE)
    out, last_end = [], 0
    for i, dot in enumerate(dots):
        if dot == 0 or dot + 6 > n:
            if "edge" not in skip or dot == 0 or dot + 1 >= n:
                continue
        if "digit_sides" not in skip and (buf[dot - 1] not in _DIGIT or buf[dot + 1] not in _DIGIT):
            continue
        start = run_of(dot)[0]          # backwards over digits and dots
        if "cursor" not in skip and start < last_end:
            continue
        end_search = min(start + 15, n)
        first = bisect.bisect_left(dots, start) if "dots_from_i" in skip else i     # dots[i..]: from the CURRENT dot
        if "dots3" not in skip and bisect.bisect_left(dots, end_search) - first < 3:
            continue
        end = _parse_ipv4(buf, start, skip)
        if end is not None:
            out.append((start, end))
            last_end = end
    return out


# ------------------------------------------------------------------------------------------------ e-mail
def model_email(buf, skip=()):
    """extract_emails_chunk / extract_email_at (lib.rs:1182-1196, 891-950) -> [(start, end)]. No cursor: every '@' stands alone."""
    buf = bytes(buf)
    n = len(buf)
    out = []
    for at in _positions(buf, b"@"):
        start = at
        while start > 0 and buf[start - 1] in EMAIL_LOCAL:
            start -= 1
        if start == at and "local_nonempty" not in skip:
            continue
        if "boundary_front" not in skip and start > 0 and buf[start - 1] not in BOUNDARY:
            continue
        end = at + 1
        while end < n and buf[end] in DOMAIN_ASCII:
            end += 1
        if end == at + 1 and "domain_nonempty" not in skip:
            continue
        if "boundary_behind" not in skip and end < n and buf[end] not in BOUNDARY:
            continue
        local, dom = buf[start:at], buf[at + 1:end]
        if "no_dotdot" not in skip and b".." in local:
            continue
        if "has_letter" not in skip and not any(c in _LETTER for c in local):
            continue
        if "domain_dot" not in skip and b"." not in dom:
            continue
        if "suffix" not in skip and find_suffix(dom) is None:
            continue
        out.append((start, end))     # (the reference's from_utf8 cannot fail: both classes are ASCII)
    return out


# ------------------------------------------------------------------------------------------------ domain
def _labels_ok(cand, min_labels, skip):
    """is_valid_domain / is_valid_label (lib.rs:637-689)"""
    labels = cand.split(b".")
    for lab in labels:
        if not lab:
            if "empty_label" not in skip:
                return False
        elif (lab[0] == 45 or lab[-1] == 45) and "hyphen" not in skip:
            return False
    return len(labels) >= min_labels or "min_labels" in skip


def model_domain(buf, min_labels=2, skip=()):
    """extract_domains_chunk_with_dots (lib.rs:537-628) -> [(start, end)]"""
    buf = bytes(buf)
    n = len(buf)
    out, last_end = [], 0
    run_of = _runs(buf, _DOMAIN_RE)
    tlds = {}
    for dot in _positions(buf, b"."):
        if "cursor" not in skip and dot < last_end:
            continue
        start, end = run_of(dot)        # backwards and forwards over is_domain_char_fast bytes
        if (start >= dot or end <= dot + 1) and "content" not in skip:
            continue
        cand = buf[start:end]
        ok = True
        if (start, end) not in tlds:    # (every dot of a run sees the same candidate)
            tlds[(start, end)] = find_suffix(cand)
        tld = tlds[(start, end)]
        if tld is None and "suffix" not in skip:
            ok = False
        elif tld == 0 and "bare" not in skip:
            ok = False
        elif "boundary_front" not in skip and start > 0 and buf[start - 1] not in BOUNDARY:
            ok = False
        elif "boundary_behind" not in skip and end < n and buf[end] not in BOUNDARY:
            ok = False
        elif not _labels_ok(cand, min_labels, skip):
            ok = False
        elif "utf8" not in skip:
            try:
                cand.decode("utf-8")
            except UnicodeDecodeError:
                ok = False
        if ok:
            out.append((start, end))
            last_end = end            # only an accept moves the cursor
        elif "accept_only" in skip:
            last_end = end
    return out


# ------------------------------------------------------------------------------------------------ hashes
def model_hashes(buf, skip=()):
    """extract_hashes_chunk_with_boundaries over find_word_boundaries_into (lib.rs:1212-1250, 1742-1782): maximal runs of
    non-boundary bytes of a hash length, all hex -> [(start, end)]. skip "boundary": maximal runs of hex digits instead."""
    buf = bytes(buf)
    out = []
    for m in (_HEXRUN_RE if "boundary" in skip else _TOKEN_RE).finditer(buf):
        s, e = m.span()
        if e - s not in HASH_TYPES and "length" not in skip:
            continue
        if "hex" not in skip and not all(c in _HEX for c in buf[s:e]):
            continue
        out.append((s, e))
    return out


def model(buf, flags=255, min_labels=2, skip=None):
    """The four types' items of extract_from_chunk in its order (lib.rs:449-485): IPv4, e-mail, domain, hashes ->
    [(type, start, end, text)], the text taken from the buffer. skip: {"ipv4" | "email" | "domain" | "hash": (rules)}"""
    buf = bytes(buf)
    skip = skip or {}
    out = []
    if flags & EX_IPV4:
        out += [("IPv4", s, e, buf[s:e].decode("ascii")) for s, e in model_ipv4(buf, skip.get("ipv4", ()))]
    if flags & EX_EMAIL:
        out += [("Email", s, e, buf[s:e].decode("ascii")) for s, e in model_email(buf, skip.get("email", ()))]
    if flags & EX_DOMAIN:
        out += [("Domain", s, e, buf[s:e].decode("utf-8", "replace")) for s, e in model_domain(buf, min_labels, skip.get("domain", ()))]
    if flags & EX_HASH:
        out += [(HASH_TYPES.get(e - s, "hex"), s, e, buf[s:e].decode("ascii", "replace")) for s, e in model_hashes(buf, skip.get("hash", ()))]
    return out


def four(items):
    """the items of an extractor that belong to this file's four extractors"""
    return [it for it in items if it[0] in FOUR_TYPES]


def verdicts(toks, items):
    """per token span the items that overlap it -> [tuple]"""
    items = sorted((s, e, t) for t, s, e, _ in items)
    starts = [s for s, _, _ in items]
    longest = max((e - s for s, e, _ in items), default=0)
    out = []
    for tok in toks:
        ts, te = tok[0], tok[1]
        lo = bisect.bisect_left(starts, ts - longest)
        hi = bisect.bisect_left(starts, te)
        out.append(tuple(it for it in items[lo:hi] if it[1] > ts and it[0] < te))
    return out


def flips(buf, toks, kind, rule, flags=255, min_labels=2):
    """the number of tokens whose verdict changes when `rule` of the `kind` model is switched off"""
    a = verdicts(toks, model(buf, flags, min_labels))
    b = verdicts(toks, model(buf, flags, min_labels, {kind: (rule,)}))
    return sum(x != y for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ generators
_LOW = b"abcdefghijklmnopqrstuvwxyz0123456789"


def _alnum(rng, n):
    return bytes(rng.choice(_LOW) for _ in range(n))


def _pack(rng, bodies, before, after, fill=None):
    """bodies between delimiters -> (buffer, [(start, end)]); no "::" arises (':' never stands in `before`)"""
    assert b":" not in before
    buf = bytearray()
    toks = []
    for body in bodies:
        a = rng.choice(before)
        if a == b"" and buf[-1:] == b":" and body[:1] == b":":
            a = b" "
        buf += a
        toks.append((len(buf), len(buf) + len(body)))
        buf += body
        buf += rng.choice(after)
        if fill is not None and rng.random() < 0.1:
            buf += fill(rng)
    buf = bytes(buf)
    assert b"::" not in buf
    return buf, toks


V4_BEFORE = [b" ", b"\n", b"/", b",", b"[", b"=", b"\"", b"(", b"@", b"x", b"Z", b".", b"", b"-", b"_", b"1", b"7", b"\xff", b"\xc3\xa9", b"\t"]
V4_AFTER = V4_BEFORE + [b":", b"]", b";"]


def _octet(rng):
    r = rng.random()
    if r < 0.62:
        return str(rng.choice([rng.randrange(256), rng.randrange(10), rng.randrange(100, 256)])).encode()
    if r < 0.70:
        return str(rng.choice([256, 260, 299, 300, 999, rng.randrange(256, 1000)])).encode()
    if r < 0.78:
        return b"0" + str(rng.randrange(100)).encode()
    if r < 0.81:
        return b""
    if r < 0.85:
        return str(rng.randrange(1000, 100000)).encode()
    return rng.choice([b"0", b"00", b"255", b"256", b"1", b"10", b"192", b"168", b"0255", b"1000"])


def ipv4_corpus(seed, count=7000):
    """-> (buffer, [(start, end)]): dotted look-alikes of 3-6 octets of 1-4 digits (values across 255 / 256, leading zeros, empty
    octets), runs such as 999.1.1.1.1 and 1.2.3.4.5, delimiters from inside and outside the boundary set (digit, '.', letter,
    high byte). The buffer ends with a quad whose first dot stands 6 bytes before the end."""
    rng = random.Random(seed * 1000003 + 4)
    bodies = []
    for _ in range(count):
        r = rng.random()
        if r < 0.45:     # a well-formed quad; the delimiters decide
            bodies.append(b".".join(str(rng.choice([rng.randrange(256), rng.randrange(10)])).encode() for _ in range(4)))
        elif r < 0.53:   # one octet wrong
            o = [str(rng.randrange(256)).encode() for _ in range(4)]
            o[rng.randrange(4)] = rng.choice([b"256", b"300", b"999", b"01", b"00", b"007", b"1234", b"", str(rng.randrange(256, 1000)).encode()])
            bodies.append(b".".join(o))
        elif r < 0.58:
            bodies.append(rng.choice([b"999.1.1.1.1", b"1.2.3.4.5", b"1.2.3.4.5.6", b"256.1.2.3.4", b"1.2.3.4.", b".1.2.3.4", b"1..2.3.4",
                                      b"1.2.3", b"1.2.3.4.5.6.7.8", b"10.0.0.1.10.0.0.2", b"0.0.0.0", b"255.255.255.255", b"1.2.3.4..5.6.7.8"]))
        else:
            bodies.append(b".".join(_octet(rng) for _ in range(rng.choice([3, 4, 4, 4, 5, 6]))))
    buf, toks = _pack(rng, bodies, V4_BEFORE, V4_AFTER)
    tail = b" 9.8.7.6"
    toks.append((len(buf) + 1, len(buf) + len(tail)))
    return buf + tail, toks


def ipv4_tail_cases():
    """quads at the end of a buffer: the first dot 6 bytes (the shortest quad's tail fits) and 5 bytes before the end, and around"""
    out = []
    for body in (b"1.2.3.4", b"12.2.3.4", b"1.2.3.", b"1.2.3", b"11.2.3", b"1.2.3.45", b"1.2.3.4 ", b"1.2.3.4x", b"1.22.3.4", b"1.2.33."):
        for head in (b"", b" ", b"x ", b"padding of some length "):
            out.append(head + body)
    return out


# distances from a dot of the name to the name's start and to its end (end - dot): both sides of every hand-over of the domain
# validators: 24 of 32 context bytes, 48 in registers, the 64-byte window, then the log itself
DOMAIN_LADDER = [6, 7, 8, 9, 23, 24, 25, 31, 32, 33, 47, 48, 49, 55, 56, 63, 64, 65, 66, 230]
DOM_TLDS = [b"com", b"net", b"org", b"io", b"co.uk", b"uk", b"ck", b"www.ck", b"za", b"co.za", b"html", b"zip", b"museum", b"photography",
            b"xn--p1ai", b"a", b"comx", b"c-m", b"", "рф".encode(), b"COM", b"travel", b"b\xc3\xbccher", b"kawasaki.jp", b"city.kawasaki.jp",
            b"x.ck", b"compute.amazonaws.com", b"blogspot.co.uk"]
DOM_DELIMS = [b" ", b"\n", b"/", b",", b"(", b")", b"\"", b"=", b";", b"<", b">", b"[", b"x", b"_", b"-", b".", b"", b"\t", b"'", b"@", b"\xff", b"!", b"+"]
_BAD_UTF8 = [b"\xc3", b"\xe2\x82", b"\xc0\xaf", b"\xe0\x80\xaf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf4\x90\x80\x80", b"\x80", b"\xff"]
_GOOD_UTF8 = ["é".encode(), "ü".encode(), "€".encode(), "рф".encode(), "😀".encode()]


def _dotted(rng, n):
    """n bytes of labels and dots that neither start nor end with a dot"""
    out = bytearray(_alnum(rng, n))
    k = rng.choice([0, 1, 2, 3, n // 8])
    for _ in range(k):
        p = rng.randrange(n)
        if 0 < p < n - 1 and out[p - 1] != 46 and out[p + 1] != 46:
            out[p] = 46
    return bytes(out)


def _ladder_name(rng, dist, side):
    """a valid name with a dot at distance `dist` from its start (side 0) or with end - dot == dist (side 1)"""
    tld = rng.choice([b"com", b"co.uk", b"org", b"io", b"museum"])
    if side == 0:
        return _dotted(rng, dist) + b"." + rng.choice([b"", _alnum(rng, rng.choice([1, 5, 20])) + b"."]) + tld
    room = dist - 1 - len(tld) - 1
    if room < 1:
        tld, room = b"io", dist - 4
    return _alnum(rng, rng.choice([1, 3, 9])) + b"." + _dotted(rng, room) + b"." + tld


def _damage(rng, name):
    """one defect somewhere in a name"""
    b = bytearray(name)
    k = rng.choice([0, 0, len(b) - 1, len(b), rng.randrange(len(b) + 1)])
    r = rng.random()
    if r < 0.35:
        b[k:k] = rng.choice(_BAD_UTF8)
    elif r < 0.50:
        b[k:k] = rng.choice(_GOOD_UTF8)
    elif r < 0.65:
        d = name.find(b".")
        b[d:d + 1] = rng.choice([b"-.", b".-", b".."])
    elif r < 0.8:
        b[k:k] = rng.choice([b"_", b"!", b"+", b"~"])
    else:
        b = bytearray(name.upper())
    return bytes(b)


def domain_corpus(seed, count=5000):
    """-> (buffer, [(start, end)]): the names of test_domain_rules_structured_fuzz, plus names with a dot at every distance of
    DOMAIN_LADDER from either end (whole and with one defect), wildcard / exception / multi-label / bare suffixes, leading and
    trailing dots, truncated and overlong UTF-8 and surrogates inside and at the ends of a name."""
    rng = random.Random(seed * 1000003 + 1)

    def label():
        r = rng.random()
        n = rng.choice([1, 1, 2, 3, 5, 8, 13, 24, 40])
        s = _alnum(rng, n)
        if r < 0.05:
            s = b"-" + s
        elif r < 0.10:
            s = s + b"-"
        elif r < 0.16:
            s = s[: n // 2] + b"-" + s[n // 2:]
        elif r < 0.19:
            s = b""
        elif r < 0.23:
            s = s + rng.choice(_GOOD_UTF8)
        elif r < 0.26:
            s = s[: n // 2] + rng.choice(_BAD_UTF8) + s[n // 2:]
        elif r < 0.30:
            s = s.upper()
        return s

    bodies = []
    for i in range(count):
        r = rng.random()
        if r < 0.55:
            k = rng.choice([0, 1, 1, 2, 2, 3, 5])
            bodies.append(b".".join([label() for _ in range(k)] + [rng.choice(DOM_TLDS)]))
        elif r < 0.90:
            name = _ladder_name(rng, DOMAIN_LADDER[i % len(DOMAIN_LADDER)], (i // len(DOMAIN_LADDER)) % 2)
            bodies.append(_damage(rng, name) if rng.random() < 0.3 else name)
        else:
            name = _alnum(rng, rng.choice([1, 4, 9])) + b"." + rng.choice([b"com", b"co.uk", b"ck", b"www.ck", b"a.b.ck", b"kawasaki.jp"])
            bodies.append(rng.choice([b".", b"", b""]) + name + rng.choice([b".", b"", b""]))
    return _pack(rng, bodies, DOM_DELIMS, DOM_DELIMS + [b":"], fill=lambda g: b"q" * g.choice([1, 7, 23, 24, 25, 100]))


# e-mail: 48 bytes in front of '@' and 32 behind it in registers, then the 80-byte window, then the log
EMAIL_LOCAL_LADDER = [0, 1, 39, 40, 41, 47, 48, 49, 80, 210]
EMAIL_DOMAIN_LADDER = [3, 4, 31, 32, 33, 39, 40, 41, 120]
EMAIL_BEFORE = [b" ", b"\n", b"<", b"=", b"\"", b"(", b",", b"x", b"_", b"\xff", b"!", b"*", b"", b"\t", b"/", b"@"]
EMAIL_AFTER = [b" ", b"\n", b">", b"\"", b")", b",", b";", b":", b"_", b"\xff", b"\xc3\xa9", b"!", b"", b"@", b"/"]


def _local(rng, n):
    if n == 0:
        return b""
    r = rng.random()
    alpha = b"0123456789" if r < 0.08 else (b"._+-" if r < 0.12 else _LOW + b"ABC")
    loc = bytearray(rng.choice(alpha) for _ in range(n))
    for _ in range(rng.choice([0, 0, 1, 3])):
        loc[rng.randrange(n)] = rng.choice(b"._+-")
    if r > 0.12 and rng.random() < 0.8:
        loc = bytearray(bytes(loc).replace(b"..", b".x"))
    if rng.random() < 0.08 and n > 2:
        k = rng.randrange(n - 1)
        loc[k:k + 2] = b".."
    return bytes(loc)


def _email_domain(rng, n):
    """a domain part of n bytes with a listed suffix (from 4 bytes on: the shortest is x.yy)"""
    if n < 4:
        return (b"a.b", b"a.", b"abc")[rng.randrange(3)][:n]
    for tld in rng.sample([b"com", b"co.uk", b"org", b"io", b"museum"], 5):
        if n - len(tld) - 1 >= 1:
            return _dotted(rng, n - len(tld) - 1) + b"." + tld
    raise AssertionError(n)


def email_corpus(seed, count=3400):
    """-> (buffer, [(start, end)]): local parts and domain parts of every length of the two ladders (and random ones), local parts
    of digits and symbols only, "..", "@@", chains, domain parts without a dot, with a numeric last label, ending in '.' or '-',
    a high byte directly behind the domain part."""
    rng = random.Random(seed * 1000003 + 2)
    bodies = []
    for i in range(count):
        nl = EMAIL_LOCAL_LADDER[i % len(EMAIL_LOCAL_LADDER)] if i % 3 else rng.choice([2, 5, 8, 13, 24])
        nd = EMAIL_DOMAIN_LADDER[(i // 3) % len(EMAIL_DOMAIN_LADDER)] if i % 3 != 1 else rng.choice([6, 9, 14, 20])
        loc, dom = _local(rng, nl), _email_domain(rng, nd)
        r = rng.random()
        if r < 0.05:
            dom = _alnum(rng, max(nd, 1))                                   # no dot
        elif r < 0.10:
            dom = _alnum(rng, 4) + b"." + rng.choice([b"123", b"7", b"nosuch", b"c-m", b"COM"])
        elif r < 0.15:
            dom += rng.choice([b".", b"-", b"..", b".-"])
        elif r < 0.19:
            bodies.append(loc + b"@" + dom + b"@" + _email_domain(rng, rng.choice([5, 9, 33])))     # a chain: two items
            continue
        elif r < 0.22:
            bodies.append(loc + b"@@" + dom)
            continue
        elif r < 0.25:
            dom = rng.choice([b"x.ck", b"www.ck", b"a.kawasaki.jp", b"city.kawasaki.jp", b"b.co.uk", b"co.uk", b"com"])
        bodies.append(loc + b"@" + dom)
    return _pack(rng, bodies, EMAIL_BEFORE, EMAIL_AFTER)


HASH_LENGTHS = [25, 26, 31, 32, 33, 39, 40, 41, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200]
HASH_BEFORE = [b" ", b"\n", b"=", b"\"", b"/", b",", b"(", b"[", b"-", b".", b"_", b"x", b"\xff", b"\t", b"  ", b" \n "]
HASH_AFTER = [b" ", b"\n", b"\"", b"/", b",", b")", b"]", b";", b":", b"-", b".", b"_", b"g", b"\xff", b"  ", b"   "]


def hash_corpus(seed, count=3000):
    """-> (buffer, [(start, end)]): hex runs of every length of HASH_LENGTHS in lower, upper and mixed case, at every start offset
    modulo 4, one non-hex byte at the first, last or a middle position, boundary and non-boundary neighbours"""
    rng = random.Random(seed * 1000003 + 3)
    bodies = []
    for i in range(count):
        n = HASH_LENGTHS[i % len(HASH_LENGTHS)] if rng.random() < 0.55 else rng.choice([32, 40, 64, 96, 128])
        alpha = rng.choice([b"0123456789abcdef", b"0123456789ABCDEF", b"0123456789abcdefABCDEF"])
        h = bytearray(rng.choice(alpha) for _ in range(n))
        r = rng.random()
        if r < 0.07:
            h[0] = rng.choice(b"gGxz_-.\xff")
        elif r < 0.14:
            h[-1] = rng.choice(b"gGxz_-.\xff")
        elif r < 0.21:
            h[rng.randrange(1, n - 1)] = rng.choice(b"gGxz_-.\xff:")
        bodies.append(bytes(h))
    heavy = lambda opts: [o for o in opts for _ in range(1 if o in (b"-", b".", b"_", b"x", b"g", b"\xff") else 2)]
    return _pack(rng, bodies, heavy(HASH_BEFORE), heavy(HASH_AFTER))


CORPORA = {"ipv4": ipv4_corpus, "domain": domain_corpus, "email": email_corpus, "hash": hash_corpus}
# the rules that can decide a verdict alone, per corpus: (model, rule, min_labels at which the floor is taken)
RULES = {
    "ipv4": [("ipv4", "cursor", 2), ("ipv4", "le255", 2), ("ipv4", "leading_zero", 2), ("ipv4", "boundary_front", 2), ("ipv4", "boundary_behind", 2)],
    "email": [("email", "boundary_front", 2), ("email", "boundary_behind", 2), ("email", "no_dotdot", 2), ("email", "has_letter", 2),
              ("email", "suffix", 2)],
    "domain": [("domain", "cursor", 2), ("domain", "suffix", 2), ("domain", "boundary_front", 2), ("domain", "boundary_behind", 2),
               ("domain", "empty_label", 2), ("domain", "hyphen", 2), ("domain", "min_labels", 3), ("domain", "utf8", 2)],
    "hash": [("hash", "length", 2), ("hash", "hex", 2), ("hash", "boundary", 2)],
}


def accepted(buf, toks, types=FOUR_TYPES):
    """the tokens that the model accepts exactly as generated -> [(start, end)]"""
    spans = {(s, e) for t, s, e, _ in model(buf) if t in types}
    return [(s, e) for s, e in toks if (s, e) in spans]


# ------------------------------------------------------------------------------------------------ edges
EDGES = [256, 2048, 2048 + 256, 6144, 8192, 16384]
_PROSE = b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et dolore magna aliqua "
H32 = b"5d41402abc4b2a76b9719d911017c592"


def edge_tokens():
    """one accept and one reject per rule of the four models -> [bytes]"""
    toks = [
        # IPv4: plain, widest, value, leading zero, too many digits, five octets, empty octet, boundaries in front and behind
        b"1.2.3.4", b"255.255.255.255", b"256.1.1.1", b"1.2.3.04", b"1.2.3.1234", b"999.1.1.1.1", b"1..2.3.4", b"x1.2.3.4", b"1.2.3.4x",
        b"\xff1.2.3.4", b"1.2.3.4-",
        # e-mail
        b"user@mail.example.org", b"u.s+e_r-1@b.co.uk", b"a@b.com@c.org", b"u..r@foo.com", b"123@foo.com", b"user@@foo.com", b"user@foo",
        b"user@foo.123", b"user@foo.com.", b"user@foo.com\xc3\xa9", b"!user@foo.com", b"user@foo.com_", b"l" * 48 + b"@" + b"d" * 28 + b".com",
        # domain
        b"evil.example.com", b"co.uk", b"foo.ck", b"foo.nosuchtld", b".foo.com", b"foo.com.", b"foo..com", b"-foo.com", b"foo-.com", b"foo.com_",
        b"caf\xc3\xa9.fr", b"caf\xc3.fr", b"a.\xed\xa0\x80.com", b"\xc0\xaffoo.com", "x.рф".encode(), b"n" * 24 + b".example.com", b"n" * 62 + b".com",
        # hashes (the longest and a 40-byte one for the long-token trigger)
        H32, H32[:-1], H32 + b"0", H32[:-1] + b"g", b"x" + H32, H32 + b"-", b"a" * 40, b"0" * 128,
    ]
    assert len(toks) == len(set(toks))
    return toks


def _filler(n):
    """n bytes of prose without '.', '@' or ':' that end with a letter"""
    out = (_PROSE * (n // len(_PROSE) + 2))[:n]
    return out[:-1] + b"e" if out.endswith(b" ") else out


def place_on_edges(tokens, edges=EDGES):
    """-> [(what, buffer)]: each token between two spaces in filler prose; every byte of the token, and the byte in front of it and
    behind it, stands in turn at offset E for every E of `edges` (one buffer holds one shift at as many edges as fit without
    overlap), and at the first and at the last byte of a buffer (the token cut there)."""
    out = []
    for tok in tokens:
        for shift in range(-1, len(tok) + 1):         # the byte at offset E is tok[shift]; -1 / len: the spaces around it
            pending = list(edges)
            while pending:
                buf = bytearray()
                rest = []
                for e in pending:
                    start = e - shift
                    if start - 1 < len(buf) + (2 if buf else 0) or start < 1:
                        rest.append(e)
                        continue
                    buf += _filler(start - 1 - len(buf))
                    buf += b" " + tok + b" "
                    assert buf[start:start + len(tok)] == tok
                assert len(rest) < len(pending), (tok, shift)
                buf += _filler(40)
                out.append(((tok, shift, tuple(e for e in pending if e not in rest)), bytes(buf)))
                pending = rest
        for k in range(len(tok)):                      # tok[k] is the first byte of a buffer / the last byte of a buffer
            out.append(((tok, k, "first"), tok[k:] + b" " + _filler(60)))
            out.append(((tok, k, "last"), _filler(60) + b" " + tok[:k + 1]))
    assert all(len(b) <= 256 * 1024 for _, b in out)
    return out


# ------------------------------------------------------------------------------------------------ IPv4 tables
def _v4(a):
    return str(ipaddress.IPv4Address(a))


def v4_table_case(seed, wide):
    """-> dict(entries=[(cidr, data)], probes=[int], text=bytes, ballot=[/24 index]). Every prefix length 9..32 (wide: 1..32; /1../8 around bases
    apart from the rest), a nested chain /8 > /16 > /17 > /23 > /24 > /25 > /31 > /32 around one base, networks whose /24 index
    is 0, 31, 32 or 63 modulo 64 with empty neighbours, and 700 distinct /24s that hold an entry longer than /24. Probes per
    sampled network: first, last, one before, one after, one inner address, written as dotted quads between delimiters."""
    rng = random.Random(seed * 31 + (1 if wide else 0))
    nets = {}

    def add(a, p):
        a &= 0xFFFFFFFF ^ ((1 << (32 - p)) - 1)
        nets.setdefault((a, p), None)

    base = (77 << 24) | (130 << 16) | (201 << 8) | 147
    for p in (8, 16, 17, 23, 24, 25, 31, 32):
        if p >= 9 or wide:
            add(base, p)
    for p in range(1 if wide else 9, 33):
        if p <= 8:
            add(0xB5A3C7E1, p)         # the wide ones nest inside 128.0.0.0/1; everything else lies below 120.0.0.0
        else:
            for _ in range(3):
                add((rng.randrange(1, 120) << 24) | rng.getrandbits(24), p)
    ballot = []
    for m in (0, 31, 32, 63):          # one ballot of k_ip_l24 covers 64 /24s: its first, middle two and last bit
        for p in (24, 27, 32):
            i24 = ((rng.randrange(1, 120) << 16) | rng.getrandbits(16)) & ~63 | m
            add((i24 << 8) | rng.getrandbits(8), p)
            ballot.append(i24)
    deep = set()
    while len(deep) < 700:             # more than the 512 leaf tables that MATCHY_AMD_LEAF_MB=1 allows
        i24 = (rng.randrange(1, 120) << 16) | rng.getrandbits(16)
        if i24 not in deep:
            deep.add(i24)
            for _ in range(rng.choice([1, 2, 4])):
                add((i24 << 8) | rng.getrandbits(8), rng.choice([25, 26, 28, 30, 31, 32, 32]))
    entries = [(f"{_v4(a)}/{p}", {"n": i, "p": p}) for i, (a, p) in enumerate(sorted(nets, key=lambda t: (t[1], t[0])))]
    sample = [k for k in nets if k[1] <= 24 or k[0] >> 8 in ballot or rng.random() < 0.25]
    probes = []
    for a, p in sample:
        size = 1 << (32 - p)
        probes += [q for q in (a, a + size - 1, a - 1, a + size, a + rng.randrange(size)) if 0 <= q <= 0xFFFFFFFF]
    for _ in range(200):
        probes.append(rng.getrandbits(32))
    probes = list(dict.fromkeys(probes))
    rng.shuffle(probes)
    text = bytearray()
    for n, q in enumerate(probes):
        text += rng.choice([b" ", b"src=", b"[", b"\"", b"(", b"from "]) + _v4(q).encode() + rng.choice([b" ", b"\n", b",", b"]", b";", b":443 "])
        if n % 8 == 7:
            text += b"\n"
    return dict(entries=entries, probes=probes, text=bytes(text), ballot=ballot)


def v4_stats(entries):
    """from the entry list alone -> (tree nodes, occupied /24s in per mille of 2^24, /24s that hold an entry longer than /24)"""
    nets = [ipaddress.ip_network(k) for k, _ in entries]
    nodes = set()
    for n in nets:
        a = int(n.network_address)
        for j in range(n.prefixlen):
            nodes.add((j, a >> (32 - j) if j else 0))
    spans = sorted((int(n.network_address) >> 8, int(n.broadcast_address) >> 8) for n in nets)
    occupied, upto = 0, -1
    for lo, hi in spans:
        lo = max(lo, upto + 1)
        if hi >= lo:
            occupied += hi - lo + 1
            upto = hi
    deep = {int(n.network_address) >> 8 for n in nets if n.prefixlen > 24}
    return len(nodes), occupied * 1000 // (1 << 24), len(deep)


# ------------------------------------------------------------------------------------------------ scans
def scan_case(seed=1):
    """-> dict(entries=[(key, data)], keys=set of text, v4=[(cidr, data)]): every fifth accepted domain, e-mail address and hash
    of the four corpora as literal keys (a third of them in upper case), and networks around every fifth accepted IPv4 address"""
    rng = random.Random(seed * 97 + 5)
    texts, quads = [], []
    for kind in ("domain", "email", "hash", "ipv4"):
        buf, _ = CORPORA[kind](seed)
        for t, s, e, v in model(buf):
            (quads if t == "IPv4" else texts).append(v)
    keys = sorted(set(texts))[::5]
    # every third ASCII key in upper case: only a case-insensitive database finds its occurrences
    keys = [k.upper() if i % 3 == 0 and k.isascii() else k for i, k in enumerate(keys)]
    nets = {}
    for q in sorted(set(quads), key=lambda v: int(ipaddress.IPv4Address(v)))[::5]:
        p = rng.choice([32, 32, 24, 16, 27, 12, 30, 9, 31, 25])
        nets.setdefault(str(ipaddress.ip_network(f"{q}/{p}", strict=False)), None)
    v4 = [(k, {"net": i}) for i, k in enumerate(nets)]
    entries = [("literal:" + k, {"n": i}) for i, k in enumerate(keys)] + v4
    return dict(entries=entries, keys=set(keys), v4=v4)


def model_hits(buf, keys, trie, case_insensitive=False):
    """what a scan reports, from the models alone -> sorted [(start, end, type, prefix length)], number of candidates"""
    fold = (lambda v: v.lower()) if case_insensitive else (lambda v: v)
    keys = {fold(k) for k in keys}
    out = []
    items = model(buf)
    for t, s, e, v in items:
        if t == "IPv4":
            r = trie.lookup(int(ipaddress.IPv4Address(v)))
            if r is not None:
                out.append((s, e, t, r[0]))
        elif fold(v) in keys:
            out.append((s, e, t, 0))
    return sorted(out), len(items)
