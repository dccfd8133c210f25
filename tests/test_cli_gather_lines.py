"""GPU: `matchy match --gather-lines` — every scanner gathers the lines with a match on the GPU and the records are rendered from that
block. The command prints the same bytes on stdout, the same [INFO] / [ERROR] lines on stderr (timings aside) and ends with the same
status as without the flag; with --gz-on-gpu the inflated text of a pack does not cross the bus."""
import gzip
import os
import re
import subprocess
from pathlib import Path

import pytest

import gz_cases as G

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 65536
TIMED = (b"[INFO] Throughput:", b"[INFO] Total time:", b"[INFO] Query rate:")


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("gather")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    plain = []
    for i in range(12):
        text = G.log(6 + 3 * i, seed=60 + i, final_newline=i % 4 != 1)
        if i == 5:
            text += b"caf\xc3\xa9 \xff 10.1.2.3 ill-formed \xe2\x82 evil.example.com\r\n"
        p = d / f"in{i:02d}.log"
        p.write_bytes(text)
        plain.append(p)
    big = d / "big.log"
    big.write_bytes(G.log(2500, seed=5))   # several batches of BATCH bytes
    gz = []
    for i in range(12):
        text = G.log(5 + 2 * i, seed=80 + i, final_newline=i % 3 != 0)
        p = d / f"rot{i:02d}.log.gz"
        # one file of two members: the GPU refuses it (trailing data) and the reader takes it the old way
        p.write_bytes(gzip.compress(text) + gzip.compress(G.log(4, seed=99)) if i == 7 else gzip.compress(text, 1 + i % 9))
        gz.append(p)
    return dbp, plain, big, gz


def _run(cli, dbp, inputs, *flags, stdin=None, env=None):
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p in inputs] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600,
                          input=stdin, env=env)


def _report(r):
    return [ln for ln in r.stderr.splitlines() if (ln.startswith(b"[INFO]") or ln.startswith(b"[ERROR]")) and not ln.startswith(TIMED)]


def same(cli, dbp, inputs, *flags, stdin=None, min_records=1, status=0):
    old = _run(cli, dbp, inputs, "-s", *flags, stdin=stdin)
    new = _run(cli, dbp, inputs, "-s", *flags, "--gather-lines", stdin=stdin)
    assert old.returncode == new.returncode == status, (old.stderr[-2000:], new.stderr[-2000:])
    assert old.stdout == new.stdout
    assert old.stdout.count(b"\n") >= min_records
    assert _report(old) == _report(new) and len(_report(old)) >= 6, (_report(old), _report(new))
    return new


def test_plain_file_of_several_batches(cli, corpus):
    dbp, plain, big, gz = corpus
    same(cli, dbp, [big], min_records=1000)
    same(cli, dbp, [big], "--devices", "0,0", min_records=1000)


def test_stdin(cli, corpus):
    dbp, plain, big, gz = corpus
    same(cli, dbp, ["-"], stdin=big.read_bytes(), min_records=1000)


def test_pack_inputs(cli, corpus):
    dbp, plain, big, gz = corpus
    new = same(cli, dbp, plain, "--pack-inputs", min_records=100)
    assert re.search(rb"\[INFO\] Packed 12 inputs into (\d+) batches", new.stderr)


def test_gz_on_gpu_with_a_file_that_falls_back(cli, corpus):
    dbp, plain, big, gz = corpus
    new = same(cli, dbp, gz, "--gz-on-gpu", min_records=100)
    assert re.search(rb"\[INFO\] Inflated 11 \.gz inputs on the GPU in (\d+) batches \((\d+) -> (\d+) bytes\), 1 read on the host", new.stderr), new.stderr[-2000:]
    assert str(gz[7]).encode() in new.stdout


def test_gz_text_stays_on_the_device(cli, corpus):
    """the trace of the gather says what crossed the bus: lines that hit, never more than the batch"""
    dbp, plain, big, gz = corpus
    r = _run(cli, dbp, gz, "--gz-on-gpu", "--gather-lines", env=dict(os.environ, MATCHY_AMD_TRACE="1"))
    assert r.returncode == 0
    rows = re.findall(rb"hit lines: (\d+) lines, block of (\d+) bytes, (\d+) bytes copied to the host", r.stderr)
    assert rows and all(a == b for _, a, b in rows)
    inflated = sum(len(gzip.decompress(p.read_bytes())) for p in gz)
    assert 0 < sum(int(b) for _, _, b in rows) < inflated


def test_line_numbers_and_input_line(cli, corpus):
    dbp, plain, big, gz = corpus
    same(cli, dbp, plain + [big], "--line-numbers", "--input-line", min_records=1000)
    same(cli, dbp, gz, "--gz-on-gpu", "--line-numbers", "--input-line", min_records=100)
    same(cli, dbp, plain, "--pack-inputs", "--line-numbers", min_records=100)


def test_format_summary(cli, corpus):
    dbp, plain, big, gz = corpus
    same(cli, dbp, plain + [big], "--format", "summary", min_records=0)
    same(cli, dbp, gz, "--gz-on-gpu", "--format", "summary", min_records=0)
