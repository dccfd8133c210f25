"""GPU: `matchy match --gz-on-gpu --gz-pieces[=BYTES]`: one large .gz among small ones prints what the run without flags prints, and the
flag alone is refused."""
import gzip
import re
import subprocess

import pytest

import gz_cases as G
import gz_pieces_cases as P
from test_cli_gz import CLI, cli   # noqa: F401  (the fixture builds the command line)

pytestmark = pytest.mark.gpu

BATCH = 2 << 20   # without --gz-pieces a member of more than 512 KiB, compressed or inflated, stays on the host


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("gz_pieces_cli")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    files = []
    for i in range(5):
        p = d / ("rot%02d.log.gz" % i)
        p.write_bytes(gzip.compress(G.log(30 + 7 * i, seed=60 + i), 1 + i))
        files.append(p)
    big = d / "access.log.gz"
    big.write_bytes(gzip.compress(P.text_1m(), 6))
    files.insert(2, big)
    return dbp, files


def run(cli, dbp, files, *flags):
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p in files] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600)


@pytest.mark.parametrize("flags", [(), ("--format", "summary"), ("--render-on-gpu",)], ids=["json", "summary", "render_on_gpu"])
def test_same_bytes_with_and_without_the_flags(cli, corpus, flags):
    dbp, files = corpus
    old = run(cli, dbp, files, "-s", *flags)
    new = run(cli, dbp, files, "-s", *flags, "--gz-on-gpu", "--gz-pieces=4096")
    assert old.returncode == new.returncode == 0, new.stderr[-3000:]
    assert old.stdout == new.stdout and (flags[:1] == ("--format",) or old.stdout.count(b"\n") > 3000)
    m = re.search(rb"\[INFO\] Inflated (\d+) \.gz inputs on the GPU in (\d+) batches \((\d+) -> (\d+) bytes\), (\d+) read on the host", new.stderr)
    assert m, new.stderr[-3000:]
    assert (int(m.group(1)), int(m.group(5))) == (len(files), 0)   # the 1 MiB file too: above a quarter of a batch, below what a pack holds


def test_default_piece_size_and_bad_values(cli, corpus):
    dbp, files = corpus
    old = run(cli, dbp, files)
    new = run(cli, dbp, files, "--gz-on-gpu", "--gz-pieces")
    assert new.returncode == 0 and old.stdout == new.stdout
    for bad in ("--gz-pieces=3", "--gz-pieces=2097152", "--gz-pieces=", "--gz-pieces=4k"):
        r = run(cli, dbp, files, "--gz-on-gpu", bad)
        assert r.returncode == 2 and b"--gz-pieces=BYTES needs a power of two" in r.stderr and r.stdout == b""


def test_the_flag_alone_is_refused(cli, corpus):
    dbp, files = corpus
    r = run(cli, dbp, files, "--gz-pieces=4096")
    assert r.returncode == 1 and b"--gz-pieces needs --gz-on-gpu" in r.stderr and r.stdout == b""
    r = run(cli, dbp, files, "--gz-on-gpu", "--gz-pieces", "--whole-lines")
    assert r.returncode == 1 and b"--whole-lines is not supported with --gz-on-gpu" in r.stderr and r.stdout == b""
