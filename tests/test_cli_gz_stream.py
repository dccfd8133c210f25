"""GPU: `matchy match --gz-on-gpu --gz-pieces=1024 --gz-stream-windows` — a .gz input of ONE member that does not fit a pack goes out as
a chain of stream windows. The command prints the same records, in the same place, and counts the same as without any gz flag; a file
whose chain ends early (no block start to land on, a wrong trailer, a cut stream) is finished by the host from the text its windows
reported. The bounds are set small (--batch-bytes, MATCHY_AMD_GZ_MAX_CARRY) so that the 200 KB of the v2_zblock vector are many windows."""
import gzip
import os
import re
import subprocess
from pathlib import Path

import pytest

import gz_cases as G
import gz_files_cases as F
import gz_stream_cases as S

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 65536
MAX_CARRY = 2048
FLAGS = ("--gz-on-gpu", "--gz-pieces=1024", "--gz-stream-windows")
STAT = rb"\[INFO\] gz stream windows on the GPU: (\d+) windows of (\d+) files, (\d+) finished on the host\n"
MODES = [(), ("--line-numbers", "--input-line"), ("--format", "summary"), ("--render-on-gpu",), ("--gather-lines",), ("--tally",)]
MODE_IDS = ["json", "line_numbers_input_line", "summary", "render_on_gpu", "gather_lines", "tally"]


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the database and the inputs in command-line order: a small .gz, the large single stream, a multi-member .gz, a plain file"""
    d = tmp_path_factory.mktemp("gzs")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    gz, text = S.vector("v2_zblock")
    assert len(gz) > BATCH and len(text) > 10 * BATCH            # it fits no pack, compressed or inflated
    files = []
    for name, data in (("small.log.gz", gzip.compress(G.log(30, seed=81))), ("big.log.gz", gz),
                       ("multi.log.gz", b"".join(F.member(G.log(20, seed=82 + k)) for k in range(3))), ("plain.log", G.log(40, seed=90))):
        (d / name).write_bytes(data)
        files.append(d / name)
    return d, dbp, files


def _run(cli, dbp, files, *flags):
    env = dict(os.environ, MATCHY_AMD_GZ_MAX_CARRY=str(MAX_CARRY))
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p in files] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600, env=env)


def _errors(r):
    # zlib names the file by its descriptor, whose number depends on what else the process has open
    return [re.sub(rb"<fd:\d+>", b"<fd>", ln) for ln in r.stderr.splitlines() if ln.startswith(b"[ERROR]")]


def _stat(r):
    m = re.search(STAT, r.stderr)
    assert m, r.stderr[-3000:]
    return tuple(map(int, m.groups()))


@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
def test_same_output_with_and_without_the_flags(cli, corpus, flags):
    """stdout is byte-identical to the run without gz flags, in the order of the command line, and the chain did the work: at least ten
    windows and no file finished on the host — without that the fallback would make every comparison pass"""
    _, dbp, files = corpus
    old = _run(cli, dbp, files, "-s", *flags)
    new = _run(cli, dbp, files, "-s", *flags, *FLAGS)
    assert old.returncode == new.returncode == 0 and _errors(old) == _errors(new) == []
    assert old.stdout == new.stdout and ("summary" in flags or old.stdout.count(b"\n") > (5 if "--tally" in flags else 3000))
    windows, n_files, on_host = _stat(new)
    assert windows >= 10 and (n_files, on_host) == (1, 0)
    counts = lambda r: re.findall(rb"\[INFO\] (?:Lines processed|Lines with matches|Total matches): ([\d,]+)", r.stderr)   # noqa: E731
    assert counts(old) == counts(new) and len(counts(old)) == 3
    if not flags:
        names = [re.search(rb'"source":"([^"]*)"', ln).group(1) for ln in new.stdout.splitlines()]
        order = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
        assert order == [str(p).encode() for p in files]        # one block per input, in command-line order
        assert b"gz stream windows" not in old.stderr


def test_chains_that_end_early_are_finished_on_the_host(cli, corpus):
    """v3_fixed has no block start to land on (NO_PROGRESS in its first window): the host reads all of it and the output is identical. A
    flipped trailer CRC, a byte of garbage behind the trailer and a stream cut in the middle fail in a window behind accepted ones: the
    [ERROR] line and the exit status are those of the run without the flag, and so are the records — except that complete lines of
    windows the GPU had accepted beyond the host's last batch cut stay reported (deviations 12 and 14)."""
    d, dbp, files = corpus
    fixed, fixed_text = S.vector("v3_fixed")
    assert len(fixed_text) > BATCH
    path = d / "fixed.log.gz"
    path.write_bytes(fixed)
    mine = [files[0], path, files[3]]
    old, new = _run(cli, dbp, mine, "-s"), _run(cli, dbp, mine, "-s", *FLAGS)
    assert old.returncode == new.returncode == 0 and old.stdout == new.stdout and old.stdout.count(b"\n") > 300
    assert _stat(new) == (0, 1, 1)
    big = files[1].read_bytes()
    bad = [m for _, m, _ in S.trailer_mutants("v2_zblock")] + [big[:len(big) // 2]]
    whole = _run(cli, dbp, [files[1]], "--line-numbers").stdout.splitlines()
    assert len(whole) > 3000
    for k, data in enumerate(bad):
        path = d / ("bad%d.log.gz" % k)
        path.write_bytes(data)
        mine = [files[0], path, files[3]]
        old, new = _run(cli, dbp, mine, "-s", "--line-numbers"), _run(cli, dbp, mine, "-s", "--line-numbers", *FLAGS)
        assert old.returncode == new.returncode and _errors(old) == _errors(new), k
        windows, n_files, on_host = _stat(new)
        assert (n_files, on_host) == (1, 1) and windows >= 5, k
        a, b = old.stdout.splitlines(), new.stdout.splitlines()
        of = lambda lines: [ln for ln in lines if path.name.encode() in ln]   # noqa: E731
        rest = lambda lines: [ln for ln in lines if path.name.encode() not in ln]   # noqa: E731
        print(f"bad{k}: rc {old.returncode} / {new.returncode}, errors {_errors(new)}, {len(of(a))} records without the flags, {len(of(b))} with them, {windows} windows")
        assert rest(a) == rest(b) and len(rest(a)) > 20, k
        # the plain run's records (the host decoder runs ahead of its batches: for a file this small it reports none), then only complete
        # lines of windows the GPU had accepted: a prefix of the records of the sound file
        assert of(b)[:len(of(a))] == of(a) and len(of(b)) > 1000, k
        assert [ln.replace(path.name.encode(), b"big.log.gz") for ln in of(b)] == whole[:len(of(b))], k
        at = b.index(of(b)[0])
        assert b[at:at + len(of(b))] == of(b), k                             # one block, at the file's place on the command line


def test_refusals(cli, corpus):
    _, dbp, files = corpus
    one = str(files[0])
    for flags in (("--gz-stream-windows",), ("--gz-stream-windows", "--gz-on-gpu"), ("--gz-stream-windows", "--gz-pieces"), ("--gz-stream-windows", "--whole-lines")):
        r = subprocess.run([cli, "match", str(dbp), one, *flags], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--gz-stream-windows needs --gz-on-gpu --gz-pieces" in r.stderr and not r.stdout, flags
    r = subprocess.run([cli, "match", str(dbp), one, *FLAGS, "--whole-lines"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--whole-lines is not supported with --gz-on-gpu" in r.stderr
    r = subprocess.run([cli, "match", str(dbp), one, *FLAGS, "--follow"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"not supported with --follow" in r.stderr
    r = subprocess.run([cli, "match"], capture_output=True, timeout=60)   # the usage text
    assert b"--gz-stream-windows" in r.stdout + r.stderr
