"""GPU: the hit tally (csrc/tally.hip, matchy_scanner_set_tally / Scanner.set_tally): matches per distinct (item type, matched text),
counted on the device from the final records of every scan and read out in count order.

The model is tests/tally_cases.py: a Counter over the ORACLE's match set of the same bytes and database, keyed by
(type, log[start:end]), put into the read-out order in Python. A read-out is compared as a whole — texts, types, counts and order."""
import ctypes
import json
import os
import re
import subprocess
import sys
from collections import Counter
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tally_cases as T   # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = T.ROOT
_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    return _hip


def on_device(data):
    dptr = ctypes.c_void_p()
    assert hip().hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(len(data) + 64)) == 0
    assert hip().hipMemcpy(dptr, data, ctypes.c_size_t(len(data)), 1) == 0
    return dptr


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


@pytest.fixture(scope="module")
def every(oracle, M):
    """the every-type log, its databases (case-sensitive and not) and the oracle's Counter for each — computed once, never modified"""
    data = T.every_type_log()
    out = {"data": data}
    for ci in (False, True):
        blob = T.build_blob(T.every_type_entries(), case_insensitive=ci)
        want, n = T.oracle_counter(oracle, blob, data)
        out[ci] = {"blob": blob, "want": want, "rows": T.ordered(want), "n": n}
    return out


def fresh(M, blob):
    db = M.Database(blob)
    sc = M.Scanner(db)
    sc.set_tally(True)
    return db, sc


def check(t, rows, what=None):
    assert list(t) == rows, what
    assert t.distinct == len(rows) and t.matches == sum(r[2] for r in rows), what


# ------------------------------------------------------------------------------------------------ 1. every type, every entry
def test_every_type_through_every_entry(M, every):
    data, e = every["data"], every[False]
    rows, n = e["rows"], e["n"]
    db = M.Database(e["blob"])
    dptr = on_device(data)

    def one(run, what, setup=None):
        sc = M.Scanner(db)
        assert not sc.tally_enabled()
        sc.set_tally(True)
        assert sc.tally_enabled()
        if setup:
            setup(sc)
        res = run(sc)
        assert res.n_hits == n, what                      # the sum of the counts is n_hits + n_ip4_hits (ScanResult.n_hits adds them)
        t = sc.tally()
        check(t, rows, what)
        res.close()
        sc.close()
        return res

    try:
        one(lambda sc: sc.scan(data), "scan")
        for mode in (0, 1, 3, 4):
            one(lambda sc: sc.scan_device(dptr.value, len(data), fetch_mode=mode), ("scan_device", mode))
        r = one(lambda sc: sc.scan_device(dptr.value, len(data), fetch_mode=9), "compact")
        assert r.n_ip4_hits > 0 and r.n_ip4_hits < n      # compact records in effect, beside 16-byte records

        def submitted(sc):
            sc.submit_device(dptr.value, len(data), fetch_mode=1)
            return sc.wait()
        one(submitted, "submit/wait")

        def sliced(sc):
            r = sc.scan_device(dptr.value, len(data), fetch_mode=1)
            assert sc.last_slices() == 3
            return r
        one(sliced, "slices", setup=lambda sc: sc.set_slices(3))
    finally:
        hip().hipFree(dptr)
    # every worker of a multi-scanner, merged on the host
    ms = M.MultiScanner(db, devices=(0, 0))
    ms.set_tally(True)
    res = ms.scan(data, batch_bytes=len(data) // 5)
    assert res.n_hits == n
    check(ms.tally(), rows, "multi")
    assert list(ms.tally(4)) == rows[:4]
    ms.reset_tally()
    t = ms.tally()
    assert list(t) == [] and t.distinct == 0 and t.matches == 0
    res.close()
    ms.close()
    db.close()


def test_case_insensitive_database_keeps_spellings_apart(M, every):
    e = every[True]
    db, sc = fresh(M, e["blob"])
    sc.scan(every["data"]).close()
    t = sc.tally()
    check(t, e["rows"])
    keys = {(typ, text) for text, typ, _ in t}
    assert {("Domain", b"evil.example.com"), ("Domain", b"Evil.Example.com"), ("Email", b"alice@test.com"), ("Email", b"Alice@test.com")} <= keys
    assert len(e["rows"]) > len(every[False]["rows"])
    sc.close(); db.close()


def test_never_enabled_and_off_mean_off(M, every):
    e = every[False]
    db = M.Database(e["blob"])
    sc = M.Scanner(db)
    plain = sc.scan(every["data"])
    hits = plain.hits()
    t = M._Tally()
    assert M.lib().matchy_scanner_tally_top(sc._h, 0, ctypes.byref(t)) == -5 and "never enabled" in M.last_error()
    with pytest.raises(RuntimeError):
        sc.tally()
    # enabled and switched off again before any scan: the table exists and is empty, scans add nothing, results are what they were
    sc.set_tally(True)
    sc.set_tally(False)
    again = sc.scan(every["data"])
    assert again.hits() == hits
    t = sc.tally()
    assert list(t) == [] and t.distinct == 0 and t.matches == 0
    sc.set_tally(True)
    with_tally = sc.scan(every["data"])
    assert with_tally.hits() == hits
    check(sc.tally(), e["rows"])
    for r in (plain, again, with_tally):
        r.close()
    sc.close(); db.close()


# ------------------------------------------------------------------------------------------------ 2. accumulation
def test_accumulation_switch_reset_and_limit(M, oracle, every):
    e = every[False]
    a = every["data"]
    b = T.every_type_log(seed=77, n_tokens=500) + b"late 203.0.113.77 10.9.1.1 10.9.1.2 10.9.1.10 fresh.bad.example.org fresh2.bad.example.org 2001:db8:1::77 ok\n"
    want_b, _ = T.oracle_counter(oracle, e["blob"], b)
    assert set(want_b) - set(e["want"])                   # B brings values A does not have
    db, sc = fresh(M, e["blob"])
    sc.scan(a).close()
    check(sc.tally(), e["rows"], "A")
    sc.scan(b).close()
    ab = e["want"] + want_b
    check(sc.tally(), T.ordered(ab), "A + B")
    n_ab = sc.tally().distinct
    sc.scan(a).close()
    aba = ab + e["want"]
    t = sc.tally()
    check(t, T.ordered(aba), "A + B + A")
    assert t.distinct == n_ab == len(ab)                  # the repeat brings no new entry
    # off: scans are not counted and the counts stay; on again: counting goes on where it was
    sc.set_tally(False)
    sc.scan(b).close()
    check(sc.tally(), T.ordered(aba), "off")
    sc.set_tally(True)
    sc.scan(b).close()
    full = T.ordered(aba + want_b)
    check(sc.tally(), full, "on again")
    # the limit cuts exactly, and ties on the count come in the stated order (type, then text)
    assert any(x[2] == y[2] and x[1] == y[1] for x, y in zip(full, full[1:])) and any(x[2] == y[2] and x[1] != y[1] for x, y in zip(full, full[1:]))
    for limit in (1, 2, 3, 5, len(full) - 1, len(full), len(full) + 7):
        t = sc.tally(limit)
        assert list(t) == full[:limit], limit
        assert t.distinct == len(full) and t.matches == sum(r[2] for r in full)
    tie = next(i for i, (x, y) in enumerate(zip(full, full[1:])) if x[2] == y[2] and x[1] == y[1])
    assert list(sc.tally(tie + 1)) == full[:tie + 1]      # a cut between two entries that differ in the text only
    sc.reset_tally()
    t = sc.tally()
    assert list(t) == [] and t.distinct == 0 and t.matches == 0 and sc.tally_enabled()
    sc.scan(a).close()
    check(sc.tally(), e["rows"], "after reset")
    sc.close(); db.close()


# ------------------------------------------------------------------------------------------------ 3 - 6: child processes
def _child(case, env):
    e = dict(os.environ)
    for k in list(e):
        if k.startswith("MATCHY_AMD_TALLY_"):
            del e[k]
    e.update(env)
    p = subprocess.run([sys.executable, str(ROOT / "tests" / "tally_cases.py"), case], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout)["steps"], p.stderr


def _model(oracle, case):
    """the expected step list of a child case: cumulative Counter after every batch"""
    entries, batches = T.CASES[case]()
    blob = T.build_blob(entries)
    total, steps = Counter(), []
    for b in batches:
        c, n = T.oracle_counter(oracle, blob, b)
        total = total + c
        steps.append({"n_hits": n, "distinct": len(total), "matches": sum(total.values()), "tally": T.rows_of(total)})
    return steps


def _trace(stderr):
    """(records, distinct, new, rehashes, pool_regrows, direct_adds) of every tally line of a child's trace"""
    return [tuple(int(x) for x in m.groups()) for m in T.TRACE_TALLY.finditer(stderr)]


def test_skew_and_the_lds_aggregator(oracle):
    want = _model(oracle, "skew")
    got, err = _child("skew", {"MATCHY_AMD_TRACE": "1"})
    assert got == want
    assert got[0]["tally"][0] == [b"10.0.0.1".hex(), "IPv4", T.SKEW_HEAVY] and got[0]["distinct"] == T.SKEW_SINGLES + 1
    (tr,) = _trace(err)
    assert tr[0] == T.SKEW_HEAVY + T.SKEW_SINGLES and tr[2] == T.SKEW_SINGLES + 1
    assert tr[5] > 0, "no count went past a workgroup's aggregator: the batch does not reach that path"


@pytest.fixture(scope="module")
def plain_run(oracle):
    want = _model(oracle, "plain")
    got, _ = _child("plain", {})
    assert got == want
    return got


@pytest.mark.parametrize("case,bits", [("collide0", 0), ("collide4", 4)])
def test_forced_hash_collisions(plain_run, case, bits):
    got, _ = _child(case, {"MATCHY_AMD_TALLY_HASH_BITS": str(bits)})
    assert got == plain_run
    assert got[0]["distinct"] >= 210


def test_growth_of_table_and_pool_with_live_counts(oracle):
    want = _model(oracle, "growth")
    got, err = _child("growth", {"MATCHY_AMD_TALLY_SLOTS": "16", "MATCHY_AMD_TALLY_POOL_BYTES": "64", "MATCHY_AMD_TRACE": "1"})
    assert got == want                                    # after every batch: the counts from before a rehash survive it
    tr = _trace(err)
    assert len(tr) == 5 and [t[2] for t in tr] == [40, 80, 160, 320, 640]
    assert tr[0][3] == 0 and all(t[3] == 1 for t in tr[1:]), tr   # the first batch sizes a new table; every later one rehashes the live table once
    # the publish pass found the pool full, the host regrew it and ran the pass again: certain in the first batch (64 bytes against 664
    # bytes of padded texts; the regrown pool holds 1328) and in the second (at least 664 + 1496 bytes by then); one regrow settles a batch
    assert tr[0][4] == 1 and tr[1][4] == 1 and all(t[4] <= 1 for t in tr), tr


def test_rescan_counts_every_hit_once(oracle):
    want = _model(oracle, "rescan")
    got, err = _child("rescan", {"MATCHY_AMD_TRACE": "1"})
    assert re.search(r"work buffers overflow \(attempt 0\): regrow and rescan:.* final_ \d+>\d+", err), err[-2000:]
    assert got == want
    assert [r[2] for r in got[0]["tally"]] == [15000] * 4
    assert len(_trace(err)) == 1                          # one tally pass for the batch, behind the last rescan


# ------------------------------------------------------------------------------------------------ 7 - 9
def test_line_context_and_tally_together(M, every):
    e = every[False]
    data = every["data"]
    db = M.Database(e["blob"])
    alone = M.Scanner(db)
    alone.set_line_context(True)
    r0 = alone.scan(data)
    lines0, lwm0, hits0 = r0.line_records, r0.lines_with_matches, r0.hits()
    both = M.Scanner(db)
    both.set_line_context(True)
    both.set_tally(True)
    r1 = both.scan(data)
    assert r1.hits() == hits0 and r1.line_records == lines0 and r1.lines_with_matches == lwm0 and lwm0 > 0
    check(both.tally(), e["rows"])
    dptr = on_device(data)
    try:
        for mode in (0, 3, 9):
            both.reset_tally()
            r = both.scan_device(dptr.value, len(data), fetch_mode=mode)
            assert r.has_lines and r.lines_with_matches == lwm0 and r.n_hits == e["n"], mode
            check(both.tally(), e["rows"], mode)
            r.close()
    finally:
        hip().hipFree(dptr)
    for r in (r0, r1):
        r.close()
    alone.close(); both.close(); db.close()


def test_ragged_end_and_empty_batch(M, oracle):
    blob = T.build_blob(T.every_type_entries())
    db, sc = fresh(M, blob)
    # the last hit ends at the last byte of the buffer, no newline behind it; a compact-record scan of the same bytes likewise
    for tail in (b"evil.example.com", b"10.1.2.3", b"2001:db8:1::5"):
        data = b"x 192.0.2.7 y\nlast line " + tail
        want, n = T.oracle_counter(oracle, blob, data)
        assert n == 2 and want[(("Domain" if b"evil" in tail else "IPv6" if b":" in tail else "IPv4"), tail)] == 1
        sc.reset_tally()
        r = sc.scan(data)
        assert r.n_hits == 2
        check(sc.tally(), T.ordered(want), tail)
        r.close()
        dptr = on_device(data)
        try:
            sc.reset_tally()
            r = sc.scan_device(dptr.value, len(data), fetch_mode=9)
            check(sc.tally(), T.ordered(want), (tail, "compact"))
            r.close()
        finally:
            hip().hipFree(dptr)
    # an empty batch and a batch without hits add nothing and break nothing
    sc.reset_tally()
    sc.scan(b"").close()
    sc.scan(b"nothing to see here\njust words\n").close()
    t = sc.tally()
    assert list(t) == [] and t.distinct == 0 and t.matches == 0
    sc.scan(b"a 192.0.2.7 b\n").close()
    sc.scan(b"").close()
    assert list(sc.tally()) == [(b"192.0.2.7", "IPv4", 1)]
    sc.close(); db.close()
