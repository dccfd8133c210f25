"""IPv6 models and generators shared by test_ipv6_host.py (CPU) and test_gpu_ipv6.py (GPU). No GPU and no project code:
the extraction model restates the reference's extract_ipv6_chunk (matchy-extractor/src/lib.rs:1044-1116, 1425-1456) with
`ipaddress.IPv6Address` as the parser, the tree model restates what a longest-prefix binary trie answers (matchy-format
mmdb/tree.rs:46-125, 258-277) from the list of entries alone. Neither looks at oracle/ or at the kernels' formulation."""
import ipaddress
import random

HEX = b"0123456789abcdefABCDEF"
_RUN = frozenset(HEX + b":")


# ------------------------------------------------------------------------------------------------ extraction model
def _linklocal_prefix(cand):
    """is_ipv6_loopback_or_linklocal (lib.rs:1425-1456)"""
    if len(cand) == 3 and cand == b"::1":
        return True
    if len(cand) >= 4:
        if cand[0:4].lower() == b"fe80":
            return True
        if cand[0:3].lower() in (b"fe8", b"fe9", b"fea", b"feb"):
            return True
    return False


def model_extract(buf):
    """extract_ipv6_chunk (lib.rs:1044-1116), line by line -> [(start, end, packed16)]"""
    buf = bytes(buf)
    out = []
    last_end = 0
    find_from = 0
    while True:
        dc = buf.find(b"::", find_from)          # memmem find_iter: matches do not overlap
        if dc < 0:
            break
        find_from = dc + 2
        if dc < last_end:
            continue
        has_hex_before = dc > 0 and buf[dc - 1] in HEX
        has_hex_after = dc + 2 < len(buf) and buf[dc + 2] in HEX
        if not has_hex_before and not has_hex_after:
            last_end = dc + 2
            continue
        start = dc
        while start > 0 and buf[start - 1] in _RUN:
            start -= 1
        end = dc + 2
        while end < len(buf) and buf[end] in _RUN:
            end += 1
        cand = buf[start:end]
        if len(cand) < 8:
            last_end = end
            continue
        if cand.startswith(b"::") or cand.endswith(b"::"):
            last_end = end
            continue
        if _linklocal_prefix(cand):
            last_end = end
            continue
        try:
            ip = ipaddress.IPv6Address(cand.decode("ascii"))
        except ValueError:
            ip = None
        if ip is not None:
            out.append((start, end, ip.packed))
            last_end = end
            continue
        last_end = dc + 2
    return out


def packed_items(items):
    """[(type, start, end, text)] of an extractor -> [(start, end, packed16)] of its IPv6 items (Rust prints ::ffff:a.b.c.d
    where Python prints hex groups: compare bytes, not text)"""
    return [(s, e, ipaddress.IPv6Address(v).packed) for t, s, e, v in items if t == "IPv6"]


# ------------------------------------------------------------------------------------------------ look-alike corpus
DELIMS = [b" ", b"\n", b"/", b",", b"[", b"]", b"=", b"\"", b"-", b"%", b"@", b".", b"x", b"g", b":", b"\xff", b""]
_FIXED = [b"fe80", b"FE9a", b"feb", b"fec0", b"ffff", b"2001", b"db8"]


def _hexgroup(rng, width):
    return bytes(rng.choice(HEX) for _ in range(width))


def _wild_group(rng):
    r = rng.random()
    if r < 0.50:
        return _hexgroup(rng, rng.randint(1, 4))
    if r < 0.62:
        return b"0" * rng.randint(1, 4)
    if r < 0.70:
        return _hexgroup(rng, 5)
    if r < 0.78:
        return b""
    return rng.choice(_FIXED)


def _join(groups, cuts, sep=b"::"):
    """groups joined with ':'; at every cut position c (0 = in front of the first group, len = behind the last) `sep` instead"""
    out = bytearray()
    n = len(groups)
    for i, g in enumerate(groups):
        if i in cuts:
            out += sep
        elif i > 0:
            out += b":"
        out += g
    if n in cuts:
        out += sep
    return bytes(out)


def token_corpus(seed, count=8000):
    """-> (buffer, [(start, end, dc_position or None)]): `count` IPv6 look-alikes packed densely between delimiters. The token
    list gives each token's body span and, for tokens with a single "::", the cut position it stands at."""
    rng = random.Random(seed)
    buf = bytearray()
    toks = []
    for _ in range(count):
        r = rng.random()
        if r < 0.40:
            # well-formed shapes: 2..7 groups of 1-4 hex digits (wide ones more often: the long accepted tokens), one inner "::"
            n = rng.choice([2, 3, 4, 5, 6, 7, 7, 7])
            wide = rng.random() < 0.45
            groups = [_hexgroup(rng, 4 if wide and rng.random() < 0.9 else rng.randint(1, 4)) for _ in range(n)]
            if rng.random() < 0.15:
                groups[rng.randrange(n)] = b"0" * rng.randint(1, 4)
            if rng.random() < 0.10:
                groups[0] = rng.choice(_FIXED)
            cut = rng.randint(1, n - 1)
            body, pos = _join(groups, {cut}), cut
        else:
            n = rng.randint(1, 9)
            groups = [_wild_group(rng) for _ in range(n)]
            k = rng.random()
            if k < 0.55:
                cut = rng.randint(0, n)                       # every cut position, first and last included
                body, pos = _join(groups, {cut}), cut
            elif k < 0.70:
                body, pos = _join(groups, set()), None        # no "::" (empty groups may still make one)
            elif k < 0.85:
                body, pos = _join(groups, {rng.randint(0, n)}, b":::"), None
            else:
                body, pos = _join(groups, {rng.randint(0, n), rng.randint(0, n)}), None
        buf += rng.choice(DELIMS)
        toks.append((len(buf), len(buf) + len(body), pos))
        buf += body
        buf += rng.choice(DELIMS)
    return bytes(buf), toks


def accepted_tokens(buf, toks):
    """the tokens of token_corpus that the model accepts exactly as generated (same span) -> [(start, end, cut position)]"""
    spans = {(s, e) for s, e, _ in model_extract(buf)}
    return [(s, e, pos) for s, e, pos in toks if (s, e) in spans]


_D1 = b"123456789"
_D4 = [b"1a2b", b"3C4d", b"5e6F", b"7081", b"92A3", b"b4c5", b"D6e7", b"f809", b"0a1B"]


def shape_tokens():
    """Deterministic enumeration: for every group count 1..8 and every "::" position (leading and trailing included) the token
    with all groups 1 digit wide and all groups 4 digits wide — the 35-byte maximum, "::" for exactly one group, eight groups
    plus "::" (rejected) — the tokens around the `len < 8` rule, and the 39-byte full form (never a candidate)."""
    out = []
    for n in range(1, 9):
        for cut in range(0, n + 1):
            out.append(_join([_D1[i:i + 1] for i in range(n)], {cut}))
            out.append(_join(_D4[:n], {cut}))
    out += [b"1::2:34", b"12::3:4", b"1::2:345", b"1:2::3:4", b"12::3:456", b"1:2::3:45", b"a::b", b"a::b:c", b"ab::c:d:e"]   # 7, 8, 9 bytes
    out.append(b":".join(_D4[:8]))
    assert len(out[-1]) == 39 and _join(_D4[:7], {3}) in out and len(_join(_D4[:7], {3})) == 35
    return out


SHAPE_WRAPS = [(b" ", b" "), (b"[", b"]"), (b"a", b" "), (b" ", b"B"), (b"c", b"D"), (b":", b" "), (b" ", b":"), (b":", b":")]


def shape_buffer():
    """every token of shape_tokens() in every wrapping, one per line"""
    buf = bytearray()
    for t in shape_tokens():
        for a, b in SHAPE_WRAPS:
            buf += b"# " + a + t + b + b" #\n"
    return bytes(buf)


# ------------------------------------------------------------------------------------------------ spellings
def spellings(addr):
    """every text form of `addr` with a "::" that neither starts nor ends it: each run of zero groups it can stand for, with
    and without leading zeros, lower and upper case"""
    addr = ipaddress.IPv6Address(addr)
    g = [int.from_bytes(addr.packed[2 * i:2 * i + 2], "big") for i in range(8)]
    out = []
    for i in range(1, 8):
        for j in range(i + 1, 8):
            if any(g[i:j]):
                continue
            for fmt in ("%x", "%04x", "%X", "%04X", None):
                def one(k, v):
                    if fmt is None:   # mixed: widths and case change from group to group
                        return ("%0*x" % (1 + (k * 7 + i) % 4, v)) if k % 2 else ("%0*X" % (1 + (k * 5 + j) % 4, v))
                    return fmt % v
                text = ":".join(one(k, g[k]) for k in range(i)) + "::" + ":".join(one(k, g[k]) for k in range(j, 8))
                if text not in out:
                    out.append(text)
    for text in out:
        assert ipaddress.IPv6Address(text) == addr and "::" in text and not text.startswith("::") and not text.endswith("::"), text
    return out


def extractable(text):
    """a spelling the extractor accepts when it stands alone between delimiters"""
    b = text.encode()
    return model_extract(b" " + b + b" ") == [(1, 1 + len(b), ipaddress.IPv6Address(text).packed)]


# ------------------------------------------------------------------------------------------------ tree model
def _v4int(text):
    return int(ipaddress.IPv4Address(text))


class TrieModel:
    """What a binary trie with one data record per entry answers, from the entries alone. entries: [(key, tag)] with key an
    IPv4 / IPv6 address or network in text; IPv4 entries stand at ::a.b.c.d/(96+p). A node exists at a path of j bits iff some
    entry is longer than j and starts with the path; the walk ends on the first record that is no node: its depth is the
    reported prefix length, its data the longest entry that contains the path — so
        prefix_len = max(p, 1 + max over entries E that do not contain the address of lcp(address, E))."""

    def __init__(self, entries):
        self.entries = []
        for key, tag in entries:
            net = ipaddress.ip_network(key, strict=True)
            if net.version == 4:
                a, p = int(net.network_address), 96 + net.prefixlen
            else:
                a, p = int(net.network_address), net.prefixlen
            self.entries.append((a, p, tag))
        self.by_len = {}
        self.nodes = [set() for _ in range(129)]
        for a, p, tag in self.entries:
            self.by_len.setdefault(p, {})[a >> (128 - p)] = tag
            for j in range(p):
                self.nodes[j].add(a >> (128 - j) if j else 0)
        self.lens = sorted(self.by_len, reverse=True)

    def _longest(self, bits, depth):
        for p in self.lens:
            if p <= depth:
                tag = self.by_len[p].get(bits >> (128 - p))
                if tag is not None:
                    return p, tag
        return None

    def _walk(self, bits, depth0, steps):
        """from the node at the first depth0 bits of `bits`, `steps` levels at most -> (levels taken, tag) | None"""
        for i in range(steps):
            j = depth0 + i + 1
            if (bits >> (128 - j)) in self.nodes[j]:   # (nodes[128] is empty: no entry is longer)
                continue
            hit = self._longest(bits, j)
            return (i + 1, hit[1]) if hit else None
        return None

    def lookup(self, addr128):
        """SearchTree::lookup_v6 in an IPv6 tree: 128 levels from the root"""
        if not self.nodes[0]:
            return None
        return self._walk(int(addr128), 0, 128)

    def formula(self, addr128):
        """the closed form of the class docstring (the tests check that it agrees with lookup())"""
        a = int(addr128)
        best, other = None, 0
        for ea, p, tag in self.entries:
            x = (a ^ ea) >> (128 - p)
            if x == 0:
                if best is None or p > best[0]:
                    best = (p, tag)
            else:
                other = max(other, p - x.bit_length())
        return (max(best[0], 1 + other), best[1]) if best else None

    def v4_chain_depth(self):
        """find_ipv4_start_node (tree.rs:258-277): left links from the root, 96 at most, for as long as they lead to nodes"""
        d = 0
        while d < 96 and 0 in self.nodes[d + 1]:
            d += 1
        return d

    def v4_lookup(self, addr32):
        """SearchTree::lookup_v4 in an IPv6 tree (tree.rs:46-90): the IPv4 bits are read from where the zero chain ends; the
        reported prefix length counts the IPv4 levels. With IPv4 entries in the tree the chain is 96 long and this is the
        ordinary answer; in an IPv6-only tree it is the `ghost` answer."""
        if not self.nodes[0]:
            return None
        d = self.v4_chain_depth()
        return self._walk(int(addr32) << (96 - d), d, 32)

    v4_in_v6only = v4_lookup

    def ghost_v4(self):
        """IPv4 addresses (ints) that an IPv6-only tree answers, one range (first, last) per reachable record"""
        d = self.v4_chain_depth()
        out = []
        for a, p, tag in self.entries:
            if p > d and (a >> (128 - d) if d else 0) == 0 and p - d <= 32:
                first = ((a << d) & ((1 << 128) - 1)) >> 96
                out.append((first, first + (1 << (32 - (p - d))) - 1))
        return out


class TrieModelV4:
    """IPv4-only tree: 32 levels. v6_in_v4tree: SearchTree::lookup_v6 walks from the root whatever the tree's version
    (tree.rs:92-125) and a 32-level tree ends there — the answer of the first 32 bits."""

    def __init__(self, entries):
        self.m = TrieModel([(str(ipaddress.ip_network(k, strict=True)), t) for k, t in entries])

    def lookup(self, addr32):
        if not self.m.nodes[0]:
            return None
        # the model keeps IPv4 entries at depth 96+p: walk the 32 levels below the (virtual) chain
        return self.m._walk(int(addr32), 96, 32)

    def v6_in_v4tree(self, addr128):
        return self.lookup(int(addr128) >> 96)


# ------------------------------------------------------------------------------------------------ tree case
def _addr_text(a):
    return str(ipaddress.IPv6Address(a))


def _v4_text(a):
    return str(ipaddress.IPv4Address(a))


def v4_entries(seed, count=3000):
    rng = random.Random(seed * 7919 + 1)
    seen, out = set(), []
    while len(out) < count:
        p = rng.choice([8, 12, 16, 20, 23, 24, 24, 24, 28, 30, 32, 32])
        a = rng.getrandbits(32) & (0xFFFFFFFF ^ ((1 << (32 - p)) - 1))
        if a >> 24 == 0 or (a, p) in seen:
            continue
        seen.add((a, p))
        out.append((f"{_v4_text(a)}/{p}", {"v4": len(out), "p": p}))
    return out


def trie_case(seed, noise_tokens=1500):
    """-> dict(entries=[(key, data)], log=bytes, probes=[address text], v6_written=[address text], v4_written=[dotted quad]).
    Entries: IPv6 networks at every prefix length 1..128 over about 40 bases with zero groups inside (so that their addresses
    have "::" spellings), among them a /16 > /32 > /48 > /64 > /96 > /127 > /128 chain. Probes per sampled network: first,
    last, one before, one after, a random inner address; every probe that has an extractable spelling stands in the log in
    1-3 spellings between random delimiters, mixed with token_corpus noise and dotted quads."""
    rng = random.Random(seed)
    full = (1 << 128) - 1
    bases = []
    while len(bases) < 40:
        g = [rng.getrandbits(16) | 1 for _ in range(8)]
        g[0] = (rng.getrandbits(16) | 0x0100) if len(bases) % 4 else (0x2001 + len(bases))
        for k in rng.sample(range(1, 7), rng.randint(1, 3)):
            g[k] = 0
        a = 0
        for v in g:
            a = (a << 16) | v
        if (a >> 112) not in {b >> 112 for b in bases} and not 0xfe80 <= (a >> 112) <= 0xfebf:
            bases.append(a)
    nets = {}

    def add(a, p):
        a &= full ^ ((1 << (128 - p)) - 1)
        nets.setdefault((a, p), None)

    for p in (16, 32, 48, 64, 96, 127, 128):
        add(bases[0], p)
    for p in range(1, 129):
        # the widest networks all around one base: the rest of the address space stays free for probes that miss
        add(bases[1] if p <= 8 else rng.choice(bases), p)
        if p > 8:
            add(rng.choice(bases[1:]), p)
    entries = [(f"{_addr_text(a)}/{p}", {"v6": i, "p": p}) for i, (a, p) in enumerate(sorted(nets, key=lambda t: (t[1], t[0])))]
    probes = []
    for a, p in nets:
        size = 1 << (128 - p)
        host = 0
        for k in range(8):
            host = (host << 16) | (0 if rng.random() < 0.4 else rng.getrandbits(16))
        cand = [a, a + size - 1, a - 1, a + size, a | (host & (size - 1))]
        probes += [c for c in cand if 0 <= c <= full]
    rng.shuffle(probes)
    probes = list(dict.fromkeys(probes))
    noise, _ = token_corpus(seed + 1000, noise_tokens)
    pieces = [noise[k:k + 4000] for k in range(0, len(noise), 4000)]
    delims = [d for d in DELIMS if d not in (b":", b"")]
    log = bytearray()
    v6_written, v4_written = [], []
    v4e = v4_entries(seed)
    for n, a in enumerate(probes):
        forms = [t for t in spellings(a) if extractable(t)]
        if forms:
            v6_written.append(_addr_text(a))
            for t in rng.sample(forms, min(len(forms), rng.randint(1, 3))):
                log += rng.choice(delims) + t.encode() + rng.choice(delims)
        if n % 3 == 0:
            key = v4e[rng.randrange(len(v4e))][0]
            net = ipaddress.ip_network(key)
            q = int(net.network_address) + rng.choice([0, net.num_addresses - 1, -1, net.num_addresses, rng.randrange(net.num_addresses)])
            q &= 0xFFFFFFFF
            v4_written.append(_v4_text(q))
            log += b" " + _v4_text(q).encode() + rng.choice([b" ", b"\n", b","])
        if n % 16 == 0:
            log += b"\n"
        if n % 40 == 0 and pieces:
            log += b"\n" + pieces.pop() + b"\n"
    return dict(entries=entries, v4_entries=v4e, log=bytes(log), probes=[_addr_text(a) for a in probes],
                v6_written=v6_written, v4_written=v4_written)
