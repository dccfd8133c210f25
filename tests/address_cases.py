"""The constructed Bitcoin / Ethereum vectors (tests/golden/btc_eth_kat.json, written by tests/golden/make_btc_eth_kat.py) and what
tests/test_oracle_kat.py and tests/test_gpu_parity.py derive from them at test time: wrappers, one-symbol mutants, batches of one
token per line and the plain-Python model of the outcome. The model is the generator's own predicates (is_btc / is_eth: the
reference's rule, lib.rs:1269-1361, 1799-1892, restated from the specifications); nothing here imports the oracle or the product.

A mutant's outcome is DECIDED BY DECODING it, never assumed: a replaced symbol may by chance give another valid token, and a
case flip may give an all-lower or all-upper Ethereum address, which is accepted without a checksum."""
import importlib.util
import json
import random
from pathlib import Path

GOLD = Path(__file__).resolve().parent / "golden"


def _generator():
    spec = importlib.util.spec_from_file_location("make_btc_eth_kat", GOLD / "make_btc_eth_kat.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
KAT = json.loads((GOLD / "btc_eth_kat.json").read_text())
XMR = json.loads((GOLD / "xmr_kat.json").read_text())

# the Monero tests' wrappers and one with the four symbols Base58 leaves out right behind the token's boundary
WRAPPERS = ((b"pay ", b" now"), (b"", b""), (b"addr=", b"\n"), (b"[", b"]"), (b"\n", b"\n"), (b"", b" 0OIl"))
B58_BAD_AT = (1, 7, 8, 15, 16, 24, 31, 32, 33)    # ... and tl - 1: both sides of every 8-byte word edge the prefilter masks


def classify(tok: str):
    """What the reference's rule makes of `tok` standing alone between word boundaries."""
    if G.is_btc(tok):
        return "Bitcoin"
    if G.is_eth(tok):
        return "Ethereum"
    return None


def accepts():
    """[(kind, text)] of every committed accept; kind is b58, bech32 or eth."""
    return ([("b58", e["text"]) for e in KAT["b58"]] + [("bech32", e["text"]) for e in KAT["bech32"]]
            + [("eth", e["text"]) for e in KAT["eth"]])


def _put(s, i, c):
    return s[:i] + c + s[i + 1:]


def _other(rng, alphabet, c):
    return rng.choice([a for a in alphabet if a != c])


def mutants():
    """{class: [text]}: every accept with one symbol of its alphabet replaced at a seeded position and at its last position; Base58
    accepts with '0', 'O', 'I', 'l' at the positions around the prefilter's word edges; Bech32 accepts with one upper-cased letter, a
    '1' and a 'b' inside the data; Ethereum accepts with the case of each letter flipped, one at a time."""
    rng = random.Random(0x6D7574)
    out = {"b58 symbol": [], "b58 outside alphabet": [], "bech32 symbol": [], "bech32 case": [], "bech32 1": [], "bech32 b": [],
           "eth symbol": [], "eth case": []}
    for kind, a in accepts():
        n = len(a)
        if kind == "b58":
            for i in (rng.randrange(n), n - 1):
                out["b58 symbol"].append(_put(a, i, _other(rng, G.ALPHABET, a[i])))
            for i in B58_BAD_AT + (n - 1,):
                if i < n:
                    out["b58 outside alphabet"] += [_put(a, i, bad) for bad in "0OIl"]
        elif kind == "bech32":
            for i in (rng.randrange(3, n), n - 1):
                out["bech32 symbol"].append(_put(a, i, _other(rng, G.BECH32_CHARSET, a[i])))
            i = rng.choice([j for j in range(3, n) if a[j].isalpha()])
            out["bech32 case"].append(_put(a, i, a[i].upper()))
            out["bech32 1"].append(_put(a, rng.randrange(3, n), "1"))
            out["bech32 b"].append(_put(a, rng.randrange(3, n), "b"))
        else:
            for i in (rng.randrange(2, n), n - 1):
                out["eth symbol"].append(_put(a, i, _other(rng, "0123456789abcdefABCDEF", a[i])))
            out["eth case"] += [_put(a, i, a[i].swapcase()) for i in range(2, n) if a[i].isalpha()]
    return out


def batch(tokens):
    """One token per line, and the (type, start, end, text) of the lines the model accepts."""
    buf, want, at = [], [], 0
    for t in tokens:
        ty = classify(t)
        if ty:
            want.append((ty, at, at + len(t), t))
        buf.append(t + "\n")
        at += len(t) + 1
    return "".join(buf).encode(), want


def coins(items):
    return [m for m in items if m[0] in ("Bitcoin", "Ethereum")]


def passes_prefix(tok: str) -> bool:
    """Whether a token reaches the checksum validators: the prefix tests in front of them (length and first characters; Base58: no
    symbol outside the alphabet among the first 64 bytes, which is every byte of a token of at most 62)."""
    n = len(tok)
    if 26 <= n <= 62 and tok.startswith("bc1"):
        return True
    if 26 <= n <= 62 and tok[0] in "13" and not any(c in tok for c in "0OIl"):
        return True
    return (n == 42 and tok.startswith("0x")) or (90 <= n <= 110 and tok[0] in "48")
