#!/usr/bin/env python3
"""Writes tests/golden/btc_eth_kat.json: checksum-VALID Bitcoin and Ethereum vectors, CONSTRUCTED from the rule.

The reference's own tests hold two Base58Check addresses (34 characters, 25-byte payloads), one Bech32 address (42 characters,
witness v0) and one mixed-case Ethereum address; tests/golden/extractor_kat.json carries those. The rule the reference applies
(crates/matchy-extractor/src/lib.rs) is much wider than the three standard address shapes, and these vectors follow the
REFERENCE'S RULE, not Bitcoin's:

  * Bitcoin (lib.rs:1269-1319): a token between word boundaries of 26..=62 bytes that
      - starts with "bc1" and for which `bech32::decode` succeeds with hrp "bc" (lib.rs:1825-1835), or
      - else starts with '1' or '3' and passes Base58Check (lib.rs:1799-1822): `bs58::decode` over the Bitcoin alphabet (a
        big-endian number; every leading '1' is one leading zero byte), decoded length >= 5, last four bytes == first four bytes
        of SHA-256(SHA-256(everything before them)). Neither the version byte nor the payload LENGTH is looked at.
  * `bech32::decode` is crate bech32 0.11. The crate's source is not available to this project, so its behaviour is RESTATED FROM
    ITS DOCUMENTATION and from BIP-173 / BIP-350: the separator is the LAST '1'; the human-readable part is 1..=83 characters
    of 33..=126; every character behind the separator is one of the 32 symbols; at least 6 of them; no mixed case; the
    checksum residue over hrp-expansion + data is 1 (Bech32) OR 0x2bc830a3 (Bech32m) — `decode` accepts either. The data need
    not be a witness program. What `decode` does with non-zero or over-long PADDING BITS when it regroups the 5-bit symbols
    into bytes is not pinned by anything here (the vectors carry random 5-bit data; oracle and kernel do not look at padding).
  * Ethereum (lib.rs:1328-1361, 1840-1892): "0x" + exactly 40 hex digits with `is_boundary_fast` bytes (or the buffer's ends)
    on both sides; all letters lower-case or all upper-case: accepted as it is; mixed case: EIP-55 — letter i is upper-case iff
    nibble i of Keccak-256(lower-case hex digits as ASCII) is >= 8 (tiny-keccak `Keccak::v256`: original 0x01 padding).

So accepts can be built: choose the payload, append the checksum, encode. Primitives: Keccak-256 is tests/golden/make_xmr_kat.py's
(pinned there by the Keccak team's vectors); SHA-256 is hashlib's; Base58 is plain integer arithmetic; the Bech32 polymod is
written from BIP-173. Pins in this script: the genesis address 1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNa for Base58Check, BIP-173's
"A12UEL5L" and BIP-350's "a1lqfn3a" for the two Bech32 constants, and the four mixed-case addresses of the EIP-55 text.

Nothing here imports the oracle or the product: the expected outcomes follow from the construction. tests/address_cases.py
derives the one-symbol mutants at test time (and decides their validity by decoding, with the predicates below).
"""
import hashlib
import json
import random
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from make_xmr_kat import ALPHABET, b58decode, b58encode, keccak256  # noqa: E402

BECH32_CHARSET = "qpzry9x8gf2tvdw0s3jn54khce6mua7l"
BECH32_CONST, BECH32M_CONST = 1, 0x2BC830A3
HEXDIGITS = "0123456789abcdef"


# ---------------------------------------------------------------------------------------------- Base58Check
def dsha4(b: bytes) -> bytes:
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()[:4]


def b58check_ok(s: str) -> bool:
    """lib.rs:1799-1822 on a string."""
    if any(ch not in ALPHABET for ch in s):
        return False
    d = b58decode(s)
    return len(d) >= 5 and dsha4(d[:-4]) == d[-4:]


def is_btc_base58(s: str) -> bool:
    return 26 <= len(s) <= 62 and s[0] in "13" and not s.startswith("bc1") and b58check_ok(s)


assert b58check_ok("1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNa") and not b58check_ok("1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNb")
assert b58decode("1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNa").hex() == "0062e907b15cbf27d5425399ebf6f0fb50ebb88f18c29b7d93"


def b58_info(s: str, cls: str) -> dict:
    """What a test needs to assert coverage: decoded (payload) length, hashed length, leading zero bytes and the number of 32-bit
    limbs the number behind them fills."""
    d = b58decode(s)
    v = int.from_bytes(d, "big")
    return {"text": s, "class": cls, "payload_len": len(d), "hashed_len": len(d) - 4, "zeros": len(d) - len(d.lstrip(b"\x00")),
            "limbs": (v.bit_length() + 31) // 32}


def b58_with_checksum(raw_wo_checksum: bytes) -> str:
    return b58encode(raw_wo_checksum + dsha4(raw_wo_checksum))


def make_b58(rng, length, first, zeros=None):
    """A Base58Check-valid token of exactly `length` characters. first == '3' (or any other non-'1' symbol): no leading zero
    byte, the number's text starts with `first`. first == '1': `zeros` leading '1' characters (default 1), then a number whose text
    does not start with '1'. The low 32 bits are replaced by the checksum; a try whose length or first digits moved is thrown away."""
    while True:
        if first == "1":
            z = zeros or 1
            digits = length - z
            v = rng.randrange(58 ** (digits - 1), 58 ** digits)      # first digit 1..57: symbol '2'..'z'
            body = b"\x00" * z + v.to_bytes((v.bit_length() + 7) // 8, "big")
        else:
            z = 0
            lo = ALPHABET.index(first) * 58 ** (length - 1)
            v = lo + rng.randrange(58 ** (length - 1))
            body = v.to_bytes((v.bit_length() + 7) // 8, "big")
        if len(body) - z < 5:
            continue
        s = b58_with_checksum(body[:-4])
        if len(s) == length and s[0] == first and (first != "1" or (s[:z] == "1" * z and s[z] != "1")):
            assert b58check_ok(s)
            return s


# ---------------------------------------------------------------------------------------------- Bech32 / Bech32m
def bech32_polymod(values):
    gen = (0x3B6A57B2, 0x26508E6D, 0x1EA119FA, 0x3D4233DD, 0x2A1462B3)
    chk = 1
    for v in values:
        top = chk >> 25
        chk = ((chk & 0x1FFFFFF) << 5) ^ v
        for i in range(5):
            if (top >> i) & 1:
                chk ^= gen[i]
    return chk


def bech32_hrp_expand(hrp):
    return [ord(c) >> 5 for c in hrp] + [0] + [ord(c) & 31 for c in hrp]


def bech32_encode(hrp, data, const):
    pm = bech32_polymod(bech32_hrp_expand(hrp) + list(data) + [0] * 6) ^ const
    return hrp + "1" + "".join(BECH32_CHARSET[d] for d in list(data) + [(pm >> 5 * (5 - i)) & 31 for i in range(6)])


def bech32_decode(s: str):
    """`bech32::decode` as restated in the docstring: (hrp, residue) or None."""
    if any(ord(c) > 126 for c in s) or (s.lower() != s and s.upper() != s) or len(s) > 1023:
        return None
    s = s.lower()
    sep = s.rfind("1")
    if sep < 1 or sep > 83 or len(s) - sep - 1 < 6 or any(ord(c) < 33 for c in s[:sep]):
        return None
    if any(c not in BECH32_CHARSET for c in s[sep + 1:]):
        return None
    return s[:sep], bech32_polymod(bech32_hrp_expand(s[:sep]) + [BECH32_CHARSET.index(c) for c in s[sep + 1:]])


def is_btc_bech32(s: str) -> bool:
    if not (26 <= len(s) <= 62 and s.startswith("bc1")):
        return False
    d = bech32_decode(s)
    return d is not None and d[0] == "bc" and d[1] in (BECH32_CONST, BECH32M_CONST)


assert bech32_decode("A12UEL5L") == ("a", BECH32_CONST) and bech32_decode("a1lqfn3a") == ("a", BECH32M_CONST)
assert bech32_decode("bc1qar0srrr7xfkvy5l643lydnw9re59gtzzwf5mdq") == ("bc", BECH32_CONST)
assert bech32_decode("bc1p5cyxnuxmeuwuvkwfem96lqzszd02n6xdcjrs20cac6yqjjwudpxqkedrcr") == ("bc", BECH32M_CONST)
assert bech32_decode("A12UEL5l") is None and bech32_decode("a1lqfn3q")[1] not in (BECH32_CONST, BECH32M_CONST)


def make_bech32(rng, length, const, hrp="bc"):
    """hrp + '1' + random 5-bit symbols + the six checksum symbols: `length` characters."""
    s = bech32_encode(hrp, [rng.randrange(32) for _ in range(length - len(hrp) - 1 - 6)], const)
    assert len(s) == length and bech32_decode(s) == (hrp, const)
    return s


def is_btc(s: str) -> bool:
    """extract_bitcoin_chunk_with_boundaries (lib.rs:1289-1317) on one whole token."""
    if not 26 <= len(s) <= 62:
        return False
    return is_btc_bech32(s) if s.startswith("bc1") else is_btc_base58(s)


# ---------------------------------------------------------------------------------------------- EIP-55
def eip55(hex40: str) -> str:
    """The checksummed spelling of 40 hex digits (EIP-55)."""
    low = hex40.lower()
    h = keccak256(low.encode()).hex()
    return "".join(c.upper() if c in "abcdef" and int(h[i], 16) >= 8 else c for i, c in enumerate(low))


def is_eth(s: str) -> bool:
    """validate_ethereum_checksum (lib.rs:1840-1892) on a whole token (the boundary rule is the caller's)."""
    if len(s) != 42 or s[:2] != "0x" or any(c not in "0123456789abcdefABCDEF" for c in s[2:]):
        return False
    letters = [c for c in s[2:] if c.isalpha()]
    if all(c.islower() for c in letters) or all(c.isupper() for c in letters):
        return True
    return eip55(s[2:]) == s[2:]


EIP55_SPEC = ["0x5aAeb6053F3E94C9b9A09f33669435E7Ef1BeAed", "0xfB6916095ca1df60bB79Ce92cE3Ea74c37c5d359",
              "0xdbF03B407c01E7cD3CBea99509d93f8DDDC8C6FB", "0xD1220A0cf47c7B9Be7A2E6BA89F429762e7b9aDb"]
for _a in EIP55_SPEC:
    assert "0x" + eip55(_a[2:]) == _a and is_eth(_a)
assert not is_eth("0x5aAeb6053F3E94C9b9A09f33669435E7Ef1BeAeD") and not is_eth("0x5AAeb6053F3E94C9b9A09f33669435E7Ef1BeAed")


def eip55_pairs(s: str):
    """(hex position, 1 if upper-case) for every letter of a mixed-case address."""
    return [(i, int(c.isupper())) for i, c in enumerate(s[2:]) if c.isalpha()]


def _digits_with_letters(rng, positions, letters):
    d = [rng.choice("0123456789") for _ in range(40)]
    for p, c in zip(positions, letters):
        d[p] = c
    return "".join(d)


# ---------------------------------------------------------------------------------------------- the file
def main():
    rng = random.Random(0x627463)
    b58, bech, eth, rejects = [], [], [], []

    # Base58Check
    for first in "13":
        for length in range(26, 63):
            b58.append(b58_info(make_b58(rng, length, first), "sweep"))
    for run in (2, 5, 14, 20, 30):
        b58.append(b58_info(make_b58(rng, 62 if run > 14 else 34 + run, "1", zeros=run), "run"))
    # the longest run of '1' in front of a number that is more than the checksum alone: one free non-zero byte + checksum is a
    # number of 6 or 7 digits, so 56 '1' when the free byte is small enough for 6 digits, else 55
    longest = None
    for z in (56, 55):
        for free in range(1, 256):
            s = b58_with_checksum(b"\x00" * z + bytes([free]))
            if len(s) <= 62 and s[z] != "1":
                longest = s
                break
        if longest:
            break
    b58.append(b58_info(longest, "run"))
    # all-zero payloads: z zero bytes are hashed; the token is z '1' (more when the checksum starts with zero bytes) + the checksum's digits
    for z in range(1, 62):
        s = b58_with_checksum(b"\x00" * z)
        if 26 <= len(s) <= 62:
            b58.append(b58_info(s, "zero"))
    assert {54, 55, 56} <= {e["hashed_len"] for e in b58 if e["class"] == "zero"}
    # 55 zero bytes and one non-zero byte: 56 hashed bytes (the first length that needs a second SHA-256 block) at 62 characters
    while True:
        s = b58_with_checksum(b"\x00" * 55 + bytes([rng.randrange(9, 256)]))
        if len(s) == 62:
            b58.append(b58_info(s, "zero+1"))
            break
    # numbers that fill 9, 10, 11 and 12 of the decoder's 32-bit limbs
    for limbs, length in ((9, 47), (10, 52), (11, 58), (12, 62)):
        while True:
            e = b58_info(make_b58(rng, length, "3"), "wide")
            if e["limbs"] == limbs:
                b58.append(e)
                break
    for e in b58:
        assert is_btc(e["text"]), e

    # Bech32 and Bech32m, random 5-bit data
    for length in range(26, 63):
        bech.append({"text": make_bech32(rng, length, BECH32_CONST), "variant": "bech32"})
        bech.append({"text": make_bech32(rng, length, BECH32M_CONST), "variant": "bech32m"})
    for e in bech:
        assert is_btc(e["text"]), e

    # Ethereum
    eth += [{"text": a, "class": "spec"} for a in EIP55_SPEC]
    seen = set()
    for a in EIP55_SPEC:
        seen |= set(eip55_pairs(a))
    while len(seen) < 80 or len(eth) < 4 + 32:     # random addresses until every (hex position, polarity) pair has occurred
        a = "0x" + eip55("".join(rng.choice(HEXDIGITS) for _ in range(40)))
        p = set(eip55_pairs(a))
        if len({q for _, q in p}) == 2:              # mixed case: the checksum is looked at
            seen |= p
            eth.append({"text": a, "class": "random"})
    base = EIP55_SPEC[0][2:]
    eth.append({"text": "0x" + base.lower(), "class": "all-lower"})
    eth.append({"text": "0x" + base.upper(), "class": "all-upper"})
    eth.append({"text": "0x" + "".join(rng.choice("0123456789") for _ in range(40)), "class": "all-digit"})
    one = _digits_with_letters(rng, [rng.randrange(40)], [rng.choice("abcdef")])
    eth.append({"text": "0x" + one, "class": "one-letter"})
    eth.append({"text": "0x" + one.upper(), "class": "one-letter"})
    while True:   # exactly two letters of which the checksum wants one upper-case and one lower-case
        two = _digits_with_letters(rng, rng.sample(range(40), 2), [rng.choice("abcdef"), rng.choice("abcdef")])
        good = eip55(two)
        if len({q for _, q in eip55_pairs("0x" + good)}) == 2:
            break
    eth.append({"text": "0x" + good, "class": "two-letters"})
    for e in eth:
        assert is_eth(e["text"]), e

    # rejects that need construction: everything but the named gate is valid
    for first in "25KLm":
        s = make_b58(rng, 34, first)
        rejects.append({"text": s, "kind": "b58", "why": f"Base58Check fine, first character {first}"})
    for length in (25, 63):
        rejects.append({"text": make_b58(rng, length, "1"), "kind": "b58", "why": f"Base58Check fine, {length} characters"})
        rejects.append({"text": make_bech32(rng, length, BECH32_CONST), "kind": "bech32", "why": f"Bech32 fine, {length} characters"})
    rejects.append({"text": make_bech32(rng, 42, BECH32_CONST, hrp="tb"), "kind": "bech32", "why": "Bech32 fine, hrp tb"})
    rejects.append({"text": "0x" + good.swapcase(), "kind": "eth", "why": "two letters, both in the wrong case"})
    rejects.append({"text": "0X" + base.lower(), "kind": "eth", "why": "0X prefix"})
    rejects.append({"text": "0x" + base.lower()[:39], "kind": "eth", "why": "39 hex digits"})
    rejects.append({"text": "0x" + base.lower() + "7", "kind": "eth", "why": "41 hex digits"})
    for r in rejects:
        assert not is_btc(r["text"]) and not is_eth(r["text"]), r
        if r["kind"] == "b58":
            assert b58check_ok(r["text"])
        if r["kind"] == "bech32":
            assert bech32_decode(r["text"])[1] == BECH32_CONST

    out = Path(__file__).with_name("btc_eth_kat.json")
    out.write_text(json.dumps({"ref": "crates/matchy-extractor/src/lib.rs:1269-1361,1799-1892", "b58": b58, "bech32": bech, "eth": eth,
                               "reject": rejects}, indent=1) + "\n")
    print(len(b58), "Base58Check,", len(bech), "Bech32 / Bech32m,", len(eth), "Ethereum accepts,", len(rejects), "rejects ->", out)


if __name__ == "__main__":
    main()
