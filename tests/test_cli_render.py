"""GPU: `matchy match --render-on-gpu` — batches whose line bases are known when they are submitted leave the device as finished
NDJSON, the others (later stream batches of a file with --line-numbers) and any batch the GPU refuses go through the host renderer.
The command prints the same bytes on stdout, the same [INFO] / [ERROR] lines on stderr (timings and the flag's own line aside) and
ends with the same status as without the flag."""
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
TIMED = (b"[INFO] Throughput:", b"[INFO] Total time:", b"[INFO] Query rate:", b"[INFO] Rendered ")
OWN = re.compile(rb"\[INFO\] Rendered (\d+) batches on the GPU \((\d+) bytes of NDJSON\), (\d+) fell back to the host renderer")


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("render")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    plain = []
    for i in range(12):
        text = G.log(6 + 3 * i, seed=60 + i, final_newline=i % 4 != 1)
        if i == 5:
            text += b"caf\xc3\xa9 \xff 10.1.2.3 \"quoted\" ill-formed \xe2\x82 evil.example.com\r\n"
        p = d / f"in{i:02d} \"q\".log"   # a source that needs escaping
        p.write_bytes(text)
        plain.append(p)
    big = d / "big.log"
    big.write_bytes(G.log(2500, seed=5))   # several batches of BATCH bytes
    gz = []
    for i in range(12):
        text = G.log(5 + 2 * i, seed=80 + i, final_newline=i % 3 != 0)
        p = d / f"rot{i:02d}.log.gz"
        if i == 7:     # two members: the GPU refuses it (trailing data) and the reader takes it the old way
            p.write_bytes(gzip.compress(text) + gzip.compress(G.log(4, seed=99)))
        elif i == 9:   # corrupt: a byte of the deflate stream flipped
            raw = bytearray(gzip.compress(text))
            raw[len(raw) // 2] ^= 0x55
            p.write_bytes(bytes(raw))
        else:
            p.write_bytes(gzip.compress(text, 1 + i % 9))
        gz.append(p)
    return dbp, plain, big, gz


def _run(cli, dbp, inputs, *flags, env=None):
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p in inputs] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600, env=env)


def _report(r):
    return [ln for ln in r.stderr.splitlines() if (ln.startswith(b"[INFO]") or ln.startswith(b"[ERROR]")) and not ln.startswith(TIMED)]


def same(cli, dbp, inputs, *flags, min_records=1, env=None):
    """(rendered on the GPU, bytes, fell back) of the run with the flag, after comparing it with the run without"""
    old = _run(cli, dbp, inputs, "-s", *flags, env=env)
    new = _run(cli, dbp, inputs, "-s", *flags, "--render-on-gpu", env=env)
    assert old.returncode == new.returncode, (old.returncode, new.returncode, old.stderr[-2000:], new.stderr[-2000:])
    assert old.stdout == new.stdout
    assert old.stdout.count(b"\n") >= min_records
    assert _report(old) == _report(new) and len(_report(old)) >= 6, (_report(old), _report(new))
    assert not OWN.search(old.stderr)
    m = OWN.search(new.stderr)
    assert m, new.stderr[-2000:]
    return tuple(int(x) for x in m.groups())


def test_plain_file(cli, corpus):
    dbp, plain, big, gz = corpus
    n, nbytes, fell = same(cli, dbp, [big], min_records=1000)
    out = _run(cli, dbp, [big]).stdout
    assert n >= 2 and fell == 0 and nbytes == len(out)   # without line numbers every batch is rendered on the GPU


def test_stream_batches_with_line_numbers_fall_back_in_the_middle(cli, corpus):
    dbp, plain, big, gz = corpus
    n, nbytes, fell = same(cli, dbp, [big, plain[3]], "--line-numbers", "--input-line", min_records=1000)
    out = _run(cli, dbp, [big, plain[3]], "--line-numbers", "--input-line").stdout
    assert 1 <= n <= 2 and fell == 0 and 0 < nbytes < len(out)   # the first batch of each input; the later batches of big.log are the host's


def test_pack_inputs(cli, corpus):
    dbp, plain, big, gz = corpus
    n, _, fell = same(cli, dbp, plain, "--pack-inputs", min_records=100)
    assert n >= 1 and fell == 0
    n, nbytes, fell = same(cli, dbp, plain, "--pack-inputs", "--line-numbers", "--input-line", min_records=100)
    out = _run(cli, dbp, plain, "--pack-inputs", "--line-numbers", "--input-line").stdout
    assert n >= 1 and fell == 0 and nbytes == len(out)   # every segment of a pack is a whole file: all of it on the GPU


def test_gz_on_gpu_with_files_the_gpu_refuses(cli, corpus):
    dbp, plain, big, gz = corpus
    for flags in ((), ("--line-numbers", "--input-line"), ("--gather-lines",)):
        n, _, fell = same(cli, dbp, gz, "--gz-on-gpu", *flags, min_records=100)
        assert n >= 1 and fell == 0
    r = _run(cli, dbp, gz, "--gz-on-gpu", "--render-on-gpu", "-s")
    assert str(gz[7]).encode() in r.stdout and r.returncode == _run(cli, dbp, gz, "--gz-on-gpu", "-s").returncode


def test_a_batch_the_renderer_refuses_falls_back(cli, corpus):
    """a byte limit below every batch's text: nothing is rendered on the GPU and the output is what it was — host batches through the
    host renderer, the members of a gz pack read the old way"""
    dbp, plain, big, gz = corpus
    env = dict(os.environ, MATCHY_AMD_RENDER_MAX_BYTES="64")
    n, _, fell = same(cli, dbp, [big], min_records=1000, env=env)
    assert n == 0 and fell >= 2
    old = _run(cli, dbp, gz, "--gz-on-gpu")
    new = _run(cli, dbp, gz, "--gz-on-gpu", "--render-on-gpu", "-s", env=env)
    # every member is then read at its place on the command line, the refused ones among them (without the fallback
    # they come behind their pack): the same records, in another order
    assert sorted(new.stdout.splitlines()) == sorted(old.stdout.splitlines()) and new.returncode == old.returncode
    n, _, fell = (int(x) for x in OWN.search(new.stderr).groups())
    assert n == 0 and fell >= 1


def test_devices_with_the_same_device_twice(cli, corpus):
    dbp, plain, big, gz = corpus
    n, _, fell = same(cli, dbp, [big] + plain, "--devices", "0,0", min_records=1000)
    assert n >= 2 and fell == 0


def test_refused_with_follow(cli, corpus):
    dbp, plain, big, gz = corpus
    r = _run(cli, dbp, [big], "--render-on-gpu", "--follow")
    assert r.returncode == 1 and b"--render-on-gpu is not supported with --follow" in r.stderr and r.stdout == b""


def test_format_summary_is_unaffected(cli, corpus):
    dbp, plain, big, gz = corpus
    old = _run(cli, dbp, plain + [big], "--format", "summary", "-s")
    new = _run(cli, dbp, plain + [big], "--format", "summary", "-s", "--render-on-gpu")
    assert old.returncode == new.returncode == 0 and old.stdout == new.stdout and _report(old) == _report(new)
    assert OWN.search(new.stderr).groups() == (b"0", b"0", b"0")
