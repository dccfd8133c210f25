"""CPU: the DEFLATE decoder rules of k_gz_inflate (matchy_amd/csrc/inflate_core.h) and the host plan (csrc/gz_plan.h), compiled with g++
under -fsanitize=address,undefined as stand-alone programs and fed every vector of tests/gz_cases.py. This run comes in front of any
GPU run of the corrupt vectors: a load behind a member's end or a store behind its capacity stops the sanitized program. No GPU."""
import struct
import subprocess
from pathlib import Path

import pytest

import gz_cases as G

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build(tmp, name):
    exe = tmp / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests" / "cpp" / (name + ".cpp")),
                    "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("inflate_core"), "test_inflate_core")


def run(driver, tmp_path, cases):
    """cases: [(gz, out_len)] -> [(status name, text or None)]"""
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    G.write_case_file(src, cases)
    r = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and "inflate_core ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    raw, pos, out = dst.read_bytes(), 0, []
    for _ in cases:
        status, n = struct.unpack_from("<iI", raw, pos)
        pos += 8
        out.append((G.STATUS[status], raw[pos:pos + n] if status == 0 else None))
        pos += n
    assert pos == len(raw)
    return out


def test_good_streams(driver, tmp_path):
    """(a) and (b): every stream inflates to zlib's bytes with status OK"""
    cases = G.good_cases()
    got = run(driver, tmp_path, [(gz, out_len) for _, gz, out_len, _, _ in cases])
    for (name, _, _, status, text), (st, t) in zip(cases, got):
        assert (st, t) == (status, text), name


def test_out_len_zero_takes_isize(driver, tmp_path):
    """out_len 0: the capacity is ISIZE, so the same streams pass without the caller's length"""
    cases = G.good_cases()
    got = run(driver, tmp_path, [(gz, 0) for _, gz, _, _, _ in cases])
    for (name, _, _, _, text), (st, t) in zip(cases, got):
        assert (st, t) == ("OK", text), name


def test_rejects(driver, tmp_path):
    """(c): every constructed reject gets the status of its rule, and zlib itself refuses the file as it stands (the two cases whose
    file is sound and whose out_len is not, aside)"""
    cases = G.reject_cases()
    got = run(driver, tmp_path, [(gz, out_len) for _, gz, out_len, _, _ in cases])
    for (name, gz, _, status, _), (st, t) in zip(cases, got):
        assert st == status and t is None, (name, st)
        if not name.endswith("_out_len"):
            assert not G.zlib_verdict(gz)[0], name


@pytest.mark.parametrize("which", [0, 1])
def test_mutants(driver, tmp_path, which):
    """(d): every single-bit flip of body and trailer, and every proper prefix: zlib decides. Rejected or not at its end -> a status
    other than OK; accepted -> OK and zlib's bytes. At least half of the flips must be rejected only after zlib has produced output."""
    name, gz, text = G.mutant_sources()[which]
    flips, cuts = list(G.bit_flips(gz)), list(G.prefixes(gz))
    verdicts = [G.zlib_verdict(m) for m in flips + cuts]
    late = sum(1 for ok, _, produced in verdicts[:len(flips)] if not ok and produced)
    print(f"{name}: {len(flips)} flips, {late} rejected after output, {sum(ok for ok, _, _ in verdicts)} accepted, {len(cuts)} prefixes")
    assert late * 2 >= len(flips)
    got = run(driver, tmp_path, [(m, len(text)) for m in flips + cuts] + [(gz, len(text))])
    assert got[-1] == ("OK", text)
    for i, ((ok, t, _), (st, out)) in enumerate(zip(verdicts, got)):
        if ok:
            assert st == "OK" and out == t, (i, st)
        else:
            assert st != "OK", i


def test_gz_plan(tmp_path):
    """csrc/gz_plan.h against the model: header parsing, starts, the separator rule, empty members, the claim order, 64-bit
    arithmetic on hostile lengths, and the refusal of a batch that reaches 2^31 bytes"""
    exe = build(tmp_path, "test_gz_plan")
    good, rej = G.good_cases(), G.reject_cases()
    members = [(gz, 0) for _, gz, _, _, _ in good] + [(gz, out_len) for _, gz, out_len, _, _ in rej] + [(b"", 0), (b"\x1f\x8b", 7), (good[0][1][:12], 0)]
    src = tmp_path / "plan.bin"
    G.write_case_file(src, members)
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [list(map(int, ln.split()[2:])) for ln in r.stdout.splitlines() if ln.startswith("member ")]
    order = [int(x) for ln in r.stdout.splitlines() if ln.startswith("order") for x in ln.split()[1:]]
    total = [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("total ")][0]
    assert len(rows) == len(members)
    start, offset, want_order = 0, 0, []
    for i, ((gz, out_len), (body, body_len, st, cap, status)) in enumerate(zip(members, rows)):
        want_status, want_cap = G.plan_status_cap(gz, out_len)
        assert (status, cap, st) == (want_status, want_cap, start), i
        if not want_status:
            hl = G.header_len(gz)
            assert (body, body_len) == (offset + hl, len(gz) - hl), i
            want_order.append(i)
        start += want_cap + 1 if want_cap else 0
        offset += len(gz)
    assert total == start
    caps = [row[3] for row in rows]
    assert order == sorted(want_order, key=lambda i: (-caps[i], i))
    # two members that vouch for 2^30 - 1 bytes each: with their separators the batch is 2^31 bytes, one byte less each and it is not
    G.write_case_file(src, [(good[0][1], (1 << 30) - 1)] * 2)
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
    G.write_case_file(src, [(good[0][1], (1 << 30) - 2)] * 2)
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0 and "total %d\n" % ((1 << 31) - 2) in r.stdout, r.stdout + r.stderr
    # ISIZE fields of 0xFFFFFFFF: 64-bit sums, refused, not wrapped
    huge = good[0][1][:-4] + b"\xff\xff\xff\xff"
    G.write_case_file(src, [(huge, 0)] * 3)
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 1 and "2^31" in r.stdout, r.stdout + r.stderr
