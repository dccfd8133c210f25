"""GPU: `matchy match --gz-on-gpu` — runs of small .gz inputs are inflated on the GPU. The command prints the same records and counts
the same as without the flag; a file the GPU does not accept is read the old way right behind its pack, so only its place in the
output moves."""
import gzip
import re
import subprocess
from pathlib import Path

import pytest

import gz_cases as G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 65536   # .gz files of up to 16384 bytes, compressed and inflated, go to the GPU; a pack holds up to 65536 bytes of text
COUNTS = [rb"\[INFO\] Files processed: ([\d,]+)", rb"\[INFO\] Files failed: ([\d,]+)", rb"\[INFO\] Lines processed: ([\d,]+)", rb"\[INFO\] Lines with matches: ([\d,]+) ",
          rb"\[INFO\] Total matches: ([\d,]+)", rb"\[INFO\] Candidates tested: ([\d,]+)"]


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the database and the inputs in command-line order: [(path, kind)] with kind plain / gz / big / multi / truncated / corrupt"""
    d = tmp_path_factory.mktemp("gz")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    files = []
    for i in range(30):
        text = G.log(5 + 2 * i, seed=40 + i, final_newline=i % 4 != 0)
        if i % 5 == 0:
            path, kind, data = d / f"plain{i:02d}.log", "plain", text
        elif i == 12:
            text = G.log(150, seed=77)
            assert len(text) > BATCH // 4
            path, kind, data = d / "big.log.gz", "big", gzip.compress(text)
        elif i == 18:
            path, kind, data = d / "multi.log.gz", "multi", gzip.compress(text) + gzip.compress(G.log(9, seed=99))
        elif i == 23:
            whole = gzip.compress(text)   # the end of the stream is gone, the trailer is there: ISIZE keeps the file eligible
            path, kind, data = d / "truncated.log.gz", "truncated", whole[:-28] + whole[-8:]
        elif i == 8:
            whole = bytearray(gzip.compress(text))   # one bit of the CRC: the reader reports it, with and without the flag
            whole[-6] ^= 0x10
            path, kind, data = d / "corrupt.log.gz", "corrupt", bytes(whole)
        elif i == 27:
            path, kind, data = d / "empty.log.gz", "gz", gzip.compress(b"")
        else:
            path, kind, data = d / f"rot{i:02d}.log.gz", "gz", gzip.compress(text, 1 + i % 9)
        path.write_bytes(data)
        files.append((path, kind))
    return dbp, files


def _run(cli, dbp, files, *flags):
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p, _ in files] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600)


def _counts(stderr):
    out = []
    for pat in COUNTS:
        m = re.search(pat, stderr)
        assert m, (pat, stderr[-3000:])
        out.append(int(m.group(1).replace(b",", b"")))
    return out


def _without(stdout, files, kinds):
    names = [str(p).encode() for p, k in files if k in kinds]
    return [ln for ln in stdout.splitlines() if not any(n in ln for n in names)]


@pytest.mark.parametrize("flags", [(), ("--line-numbers", "--input-line"), ("--pack-inputs",), ("--devices", "0,0")],
                         ids=["json", "line_numbers_input_line", "pack_inputs", "two_scanners"])
def test_same_records_with_and_without_the_flag(cli, corpus, flags):
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", *flags)
    new = _run(cli, dbp, files, "-s", *flags, "--gz-on-gpu")
    assert old.returncode == new.returncode == 1   # the corrupt file
    assert old.stdout.count(b"\n") > 400
    assert sorted(old.stdout.splitlines()) == sorted(new.stdout.splitlines())
    # as sequences, the files that fall back aside: they are the ones whose records move behind their pack
    fallen = ("multi", "truncated", "corrupt")
    assert _without(old.stdout, files, fallen) == _without(new.stdout, files, fallen)
    assert any(str(p).encode() in old.stdout for p, k in files if k == "multi")
    bad = str([p for p, k in files if k == "corrupt"][0]).encode()
    err = lambda r: [ln for ln in r.stderr.splitlines() if ln.startswith(b"[ERROR]")]   # noqa: E731
    assert err(old) == err(new) and len(err(old)) == 1 and bad in err(old)[0]
    assert _counts(old.stderr) == _counts(new.stderr)
    n_gz = sum(1 for _, k in files if k == "gz")
    m = re.search(rb"\[INFO\] Inflated (\d+) \.gz inputs on the GPU in (\d+) batches \((\d+) -> (\d+) bytes\), (\d+) read on the host", new.stderr)
    assert m, new.stderr[-3000:]
    n, batches, packed, text, host = map(int, m.groups())
    assert (n, host) == (n_gz, 3) and batches >= 4   # runs between the plain files and the big one; three files fall back
    assert packed == sum(p.stat().st_size for p, k in files if k == "gz")
    assert text == sum(len(gzip.decompress(p.read_bytes())) for p, k in files if k == "gz")
    assert b"Inflated" not in old.stderr


def test_summary_counts_are_equal(cli, corpus):
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", "--format", "summary")
    new = _run(cli, dbp, files, "-s", "--format", "summary", "--gz-on-gpu")
    assert old.returncode == new.returncode == 1
    assert old.stdout == new.stdout
    assert _counts(old.stderr) == _counts(new.stderr) and _counts(old.stderr)[4] > 400


def test_tally_is_equal(cli, corpus):
    dbp, files = corpus
    old = _run(cli, dbp, files, "--format", "summary", "--tally=0")
    new = _run(cli, dbp, files, "--format", "summary", "--tally=0", "--gz-on-gpu")
    assert old.stdout == new.stdout and old.stdout.count(b"\n") > 10


def test_member_bound_from_the_environment(cli, corpus):
    """MATCHY_AMD_GZ_MAX_MEMBER lowers the bound: with 19 bytes (the empty file has 20) nothing is eligible and nothing goes to the GPU
    compressed"""
    import os
    dbp, files = corpus
    assert min(p.stat().st_size for p, k in files if k != "plain") == 20
    env = dict(os.environ, MATCHY_AMD_GZ_MAX_MEMBER="19")
    new = subprocess.run([cli, "match", str(dbp)] + [str(p) for p, _ in files] + ["--batch-bytes", str(BATCH), "-s", "--gz-on-gpu"], capture_output=True, timeout=600, env=env)
    old = _run(cli, dbp, files, "-s")
    assert new.stdout == old.stdout
    assert re.search(rb"Inflated 0 \.gz inputs on the GPU in 0 batches \(0 -> 0 bytes\), 0 read on the host", new.stderr)


def test_follow_is_refused(cli, corpus):
    dbp, files = corpus
    r = subprocess.run([cli, "match", str(dbp), str(files[1][0]), "--gz-on-gpu", "--follow"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--gz-on-gpu is not supported with --follow" in r.stderr
