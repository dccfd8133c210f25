"""CPU: the host side of the hit tally — the C ABI surface (header, export list, library, Python mirror), the null-handle behaviour, the
layout and read-out logic the host shares with the kernels (csrc/tally.h) run alone under AddressSanitizer + UBSan, and the inputs of
the GPU tests: every constructed log must yield, from the oracle, the hits its case is about."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tally_cases as T   # noqa: E402

ROOT = T.ROOT

NEW_FUNCTIONS = ["matchy_scanner_set_tally", "matchy_scanner_tally", "matchy_scanner_reset_tally", "matchy_scanner_tally_top",
                 "matchy_multi_scanner_set_tally", "matchy_multi_scanner_tally_top", "matchy_multi_scanner_reset_tally", "matchy_tally_free"]


def test_header_export_list_library_and_mirror_carry_the_tally_calls():
    import ctypes as C
    import matchy_amd as M
    header = (ROOT / "include" / "matchy_amd.h").read_text()
    L = M.lib()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in M.EXPORTED_SYMBOLS, name
        assert getattr(L, name) is not None
    assert re.search(r"int32_t\s+matchy_scanner_tally_top\s*\(\s*matchy_scanner_t\s*\*\s*\w*,\s*size_t\s+\w+,\s*matchy_tally_t\s*\*", header)
    assert re.search(r"typedef struct matchy_tally_entry_t \{ const uint8_t \*text; uint32_t len; uint8_t item_type; uint64_t count; \}", header)
    assert re.search(r"typedef struct matchy_tally_t \{ const matchy_tally_entry_t \*entries; size_t n_entries; uint64_t distinct, matches; void \*_internal; \}", header)
    # the mirror's structures have the C layout (x86-64: 8 + 4 + 1 + pad + 8, and five words)
    assert C.sizeof(M._TallyEntry) == 24 and M._TallyEntry.count.offset == 16 and M._TallyEntry.item_type.offset == 12
    assert C.sizeof(M._Tally) == 40
    # a null handle is harmless
    L.matchy_scanner_set_tally(None, True)
    L.matchy_scanner_reset_tally(None)
    assert not L.matchy_scanner_tally(None)
    t = M._Tally()
    assert L.matchy_scanner_tally_top(None, 3, C.byref(t)) == -5 and L.matchy_multi_scanner_tally_top(None, 3, C.byref(t)) == -5   # MATCHY_ERROR_INVALID_PARAM
    assert L.matchy_multi_scanner_set_tally(None, True) == -5
    L.matchy_multi_scanner_reset_tally(None)
    L.matchy_tally_free(None)
    L.matchy_tally_free(C.byref(t))   # an empty one
    for cls in (M.Scanner, M.MultiScanner):
        for attr in ("set_tally", "reset_tally", "tally"):
            assert hasattr(cls, attr), (cls, attr)


def test_sources_build_list_and_command_line():
    import matchy_amd.build as B
    assert "tally.hip" in B.SOURCES
    src = "".join((ROOT / "matchy_amd" / "csrc" / name).read_text() for name in [*B.CLI_SOURCES, "gz_packer.h"])   # the command line
    assert "--tally" in src and "matchy_multi_scanner_tally_top" in src
    hip = (ROOT / "matchy_amd" / "csrc" / "tally.hip").read_text()
    for k in ("k_tally_claim", "k_tally_publish", "k_tally_export", "k_tally_gather"):
        assert re.search(r"__global__[^;{]*\b%s\b" % k, hip), k
    # the rehash kernel is the text table's, shared with the distinct-text set
    assert "text_table.hip" in B.SOURCES and re.search(r"__global__[^;{]*\bk_text_rehash\b", (ROOT / "matchy_amd" / "csrc" / "text_table.hip").read_text())
    for env in ("MATCHY_AMD_TALLY_SLOTS", "MATCHY_AMD_TALLY_POOL_BYTES", "MATCHY_AMD_TALLY_HASH_BITS"):
        assert env in hip


def test_layout_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "test_tally_layout"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests/cpp/test_tally_layout.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tally layout: ok" in r.stdout


def test_ordered_is_the_stated_order():
    from collections import Counter
    c = Counter({("Domain", b"b.example.com"): 2, ("Domain", b"a.example.com"): 2, ("IPv4", b"10.0.0.1"): 2, ("IPv6", b"::1"): 2, ("Domain", b"zz.example.com"): 5,
                 ("Domain", b"a.example.co"): 2, ("MD5", b"f" * 32): 2, ("SHA1", b"0" * 40): 2, ("Email", b"a@b.com"): 1})
    assert [r[0] for r in T.ordered(c)] == [b"zz.example.com", b"::1", b"10.0.0.1", b"a.example.co", b"a.example.com", b"b.example.com", b"0" * 40, b"f" * 32, b"a@b.com"]


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
@pytest.mark.parametrize("ci", [False, True])
def test_every_type_log_hits_every_class(oracle, ci):
    data = T.every_type_log()
    assert 3 * 8192 <= len(data) <= 64 << 10 and 200 <= data.count(b"\n") <= 900   # a few hundred lines, long enough for three slices
    want, n = T.oracle_counter(oracle, T.build_blob(T.every_type_entries(), case_insensitive=ci), data)
    types = {t for t, _ in want}
    assert {"IPv4", "IPv6", "Domain", "Email", "MD5", "SHA256", "Bitcoin", "Ethereum", "Monero"} <= types, types
    btc, eth, xmr = T.golden_addresses()
    for key in [("IPv4", b"192.0.2.7"), ("IPv4", b"10.1.2.3"), ("IPv4", b"10.9.8.7"), ("IPv6", b"2001:db8:1::5"), ("IPv6", b"2001:DB8:1::5"), ("IPv6", b"2001:db8:ffff::1"),
                ("Domain", b"evil.example.com"), ("Domain", b"www.bad.example.org"), ("Domain", b"cdn-7.example.net"), ("Email", b"alice@test.com"),
                ("Email", b"bob@mail.example.net"), ("MD5", T.MD5.encode()), ("SHA256", T.SHA256.encode()), ("Bitcoin", btc.encode()), ("Ethereum", eth.encode()),
                ("Monero", xmr.encode())]:
        assert want[key] >= 2, key
    for miss in [("IPv4", b"203.0.113.5"), ("Domain", b"good.example.com"), ("Email", b"carol@test.com"), ("MD5", b"a" * 32), ("IPv6", b"2001:db8:2::1")]:
        assert miss not in want, miss
    # texts that differ only in letter case: the case-insensitive database hits both spellings, and they stay two keys
    for key in [("Domain", b"Evil.Example.com"), ("Email", b"Alice@test.com"), ("MD5", T.MD5.upper().encode())]:
        assert (want[key] >= 2) == ci, (key, ci)
    assert sum(want.values()) == n and len(want) > 22   # more values than the command line's default report of 20 rows
    # ties on the count exist, so the order's later keys matter
    counts = [c for _, _, c in T.ordered(want)]
    assert len(set(counts)) < len(counts)


def test_child_cases_hit_what_they_are_about(oracle):
    entries, (batch,) = T.CASES["plain"]()
    want, n = T.oracle_counter(oracle, T.build_blob(entries), batch)
    assert len(want) >= 210 and n >= 600 and {"IPv4", "Domain", "IPv6", "Email", "MD5", "Bitcoin"} <= {t for t, _ in want}
    # growth: every batch brings new values and repeats old ones
    entries, batches = T.CASES["growth"]()
    blob, seen = T.build_blob(entries), set()
    for k, b in enumerate(batches):
        c, _ = T.oracle_counter(oracle, blob, b)
        new = set(c) - seen
        assert len(new) == (40, 80, 160, 320, 640)[k] and (k == 0 or len(set(c) & seen) >= 10), k
        seen |= set(c)
    assert {t for t, _ in seen} == {"IPv4", "Domain"}
    # rescan: more records than a fresh scanner's final list holds (tests/test_gpu_overflow.py initial_caps: max(1024, max(4096, len // 24) // 4))
    entries, (batch,) = T.CASES["rescan"]()
    want, n = T.oracle_counter(oracle, T.build_blob(entries), batch)
    assert n == 60000 and n > max(1024, max(4096, len(batch) // 24) // 4) and sorted(want.values()) == [15000] * 4


def test_skew_batch(oracle):
    entries, (batch,) = T.CASES["skew"]()
    want, n = T.oracle_counter(oracle, T.build_blob(entries), batch)
    assert n == T.SKEW_HEAVY + T.SKEW_SINGLES and want[("IPv4", b"10.0.0.1")] == T.SKEW_HEAVY
    assert len(want) == T.SKEW_SINGLES + 1 and sorted(want.values())[-2] == 1
    # the singles stand in runs of SKEW_CLUMP consecutive lines, more than the 256 entries of a workgroup's aggregator
    lines = batch.split(b"\n")
    run = best = 0
    for ln in lines:
        run = run + 1 if ln and ln != b"10.0.0.1" else 0
        best = max(best, run)
    assert best == T.SKEW_CLUMP > 256
