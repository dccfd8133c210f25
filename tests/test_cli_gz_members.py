"""GPU: `matchy match --gz-on-gpu --gz-members` — .gz inputs of many members that fit one pack are inflated on the GPU, one wave per
member. The command prints the same records and counts the same as without the flags; a file the GPU does not accept is read the old
way right behind its pack, so only its place in the output moves. The corpus is that of tests/test_cli_gz.py plus four files."""
import gzip
import re
import subprocess
from pathlib import Path

import pytest

import gz_cases as G
import gz_files_cases as F

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 65536
COUNTS = [rb"\[INFO\] Files processed: ([\d,]+)", rb"\[INFO\] Files failed: ([\d,]+)", rb"\[INFO\] Lines processed: ([\d,]+)", rb"\[INFO\] Lines with matches: ([\d,]+) ",
          rb"\[INFO\] Total matches: ([\d,]+)", rb"\[INFO\] Candidates tested: ([\d,]+)"]
MULTI_OK = ("multi", "m40", "bgzf")                       # files of many members the GPU accepts
FALLEN = ("truncated", "corrupt", "mcorrupt")             # eligible, refused by the GPU, read the old way behind their pack


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the database and the inputs in command-line order: [(path, kind)]"""
    d = tmp_path_factory.mktemp("gzm")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    files = []

    def put(name, kind, data):
        (d / name).write_bytes(data)
        files.append((d / name, kind))
    for i in range(30):
        text = G.log(5 + 2 * i, seed=40 + i, final_newline=i % 4 != 0)
        if i % 5 == 0:
            put(f"plain{i:02d}.log", "plain", text)
        elif i == 12:
            text = G.log(150, seed=77)
            assert len(text) > BATCH // 4
            put("big.log.gz", "big", gzip.compress(text))
        elif i == 18:
            put("multi.log.gz", "multi", gzip.compress(text) + gzip.compress(G.log(9, seed=99)))
        elif i == 23:
            whole = gzip.compress(text)
            put("truncated.log.gz", "truncated", whole[:-28] + whole[-8:])
        elif i == 8:
            whole = bytearray(gzip.compress(text))
            whole[-6] ^= 0x10
            put("corrupt.log.gz", "corrupt", bytes(whole))
        elif i == 27:
            put("empty.log.gz", "gz", gzip.compress(b""))
        else:
            put(f"rot{i:02d}.log.gz", "gz", gzip.compress(text, 1 + i % 9))
        if i == 3:     # 40 members, some without a final newline: lines span members
            put("m40.log.gz", "m40", b"".join(F.member(G.log(1 + k % 4, seed=300 + k, final_newline=k % 3 != 0), 1 + k % 9) for k in range(40)))
        elif i == 13:  # BGZF-style: cut mid-line, the empty block last
            put("bgzf.log.gz", "bgzf", F.bgzf_file(G.log(70, seed=310), 1500))
        elif i == 21:  # the third of four members has a flipped CRC bit
            parts = [bytearray(F.member(G.log(6 + k, seed=320 + k))) for k in range(4)]
            parts[2][-6] ^= 0x10
            put("mcorrupt.log.gz", "mcorrupt", b"".join(bytes(p) for p in parts))
        elif i == 25:  # more text than a pack holds
            data = b"".join(F.member(G.log(80, seed=330 + k)) for k in range(7))
            assert len(gzip.decompress(data)) > BATCH
            put("mbig.log.gz", "mbig", data)
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


def _members(path):
    return len(F.split_members(path.read_bytes()))


@pytest.mark.parametrize("flags", [(), ("--line-numbers", "--input-line"), ("--pack-inputs",), ("--render-on-gpu", "--gather-lines")],
                         ids=["json", "line_numbers_input_line", "pack_inputs", "render_on_gpu_gather_lines"])
def test_same_records_with_and_without_the_flags(cli, corpus, flags):
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", *flags)
    new = _run(cli, dbp, files, "-s", *flags, "--gz-on-gpu", "--gz-members")
    assert old.returncode == new.returncode == 1   # the corrupt files
    assert old.stdout.count(b"\n") > 600
    assert sorted(old.stdout.splitlines()) == sorted(new.stdout.splitlines())
    assert _without(old.stdout, files, FALLEN) == _without(new.stdout, files, FALLEN)
    for kind in MULTI_OK + ("mbig",):
        assert any(str(p).encode() in old.stdout for p, k in files if k == kind), kind
    err = lambda r: sorted(ln for ln in r.stderr.splitlines() if ln.startswith(b"[ERROR]"))   # noqa: E731
    assert err(old) == err(new) and len(err(old)) == 2
    assert _counts(old.stderr) == _counts(new.stderr)
    on_gpu = [p for p, k in files if k == "gz" or k in MULTI_OK]
    m = re.search(rb"\[INFO\] Inflated (\d+) \.gz inputs on the GPU in (\d+) batches \((\d+) -> (\d+) bytes\), (\d+) read on the host\n"
                  rb"\[INFO\] gz members on the GPU: (\d+) in (\d+) multi-member files\n", new.stderr)
    assert m, new.stderr[-3000:]
    n, batches, packed, text, host, n_members, n_multi = map(int, m.groups())
    assert (n, host) == (len(on_gpu), len(FALLEN)) and batches >= 4
    assert packed == sum(p.stat().st_size for p in on_gpu)
    assert text == sum(len(gzip.decompress(p.read_bytes())) for p in on_gpu)
    multi = [p for p, k in files if k in MULTI_OK]
    assert (n_members, n_multi) == (sum(_members(p) for p in multi), 3) and n_members > 45
    assert b"Inflated" not in old.stderr and b"gz members" not in old.stderr


def test_summary_counts_and_tally_are_equal(cli, corpus):
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0")
    new = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0", "--gz-on-gpu", "--gz-members")
    assert old.returncode == new.returncode == 1
    assert old.stdout == new.stdout and old.stdout.count(b"\n") > 10
    assert _counts(old.stderr) == _counts(new.stderr) and _counts(old.stderr)[4] > 600
    assert b"gz members on the GPU: " in new.stderr


def test_without_the_flag_multi_member_files_stay_on_the_host(cli, corpus):
    """--gz-on-gpu alone: every file of more than one member that is small enough to be tried comes back with TRAILING_DATA and is read
    on the host; no second statistics line"""
    dbp, files = corpus
    r = _run(cli, dbp, files, "-s", "--gz-on-gpu")
    m = re.search(rb"\[INFO\] Inflated (\d+) \.gz inputs on the GPU in \d+ batches \(\d+ -> \d+ bytes\), (\d+) read on the host", r.stderr)
    assert m, r.stderr[-3000:]
    tried = [p for p, k in files if k in MULTI_OK + FALLEN + ("mbig",) and p.stat().st_size <= BATCH // 4 and int.from_bytes(p.read_bytes()[-4:], "little") <= BATCH // 4]
    assert int(m.group(1)) == sum(1 for _, k in files if k == "gz") and int(m.group(2)) == len(tried) >= 6
    assert b"gz members" not in r.stderr


def test_refusals(cli, corpus):
    dbp, files = corpus
    one = str(files[1][0])
    r = subprocess.run([cli, "match", str(dbp), one, "--gz-members"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--gz-members needs --gz-on-gpu" in r.stderr
    r = subprocess.run([cli, "match", str(dbp), one, "--gz-on-gpu", "--gz-members", "--follow"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"not supported with --follow" in r.stderr
    r = subprocess.run([cli, "match", str(dbp), one, "--gz-on-gpu", "--gz-members", "--whole-lines"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--whole-lines is not supported with --gz-on-gpu" in r.stderr
