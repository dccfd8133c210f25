"""GPU: `matchy match --pack-inputs` — consecutive small files share a batch and are told apart on the GPU; the command prints byte
for byte what it prints without the flag, and counts the same."""
import gzip
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 16384   # files of up to 4096 bytes are packed


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


def _lines(i, n, crlf=False):
    out = []
    for k in range(n):
        if (i + k) % 4 == 0:
            out.append(b"GET /p%d from 10.1.2.%d to evil.example.com status ok" % (k, (i * 7 + k) % 250))
        elif (i + k) % 9 == 2:
            out.append(b"host 192.0.2.7 asked www.bad.example.org")
        elif (i + k) % 5 == 1:
            out.append(b"")
        else:
            out.append(b"nothing to see in line %d of file %d, only filler text" % (k, i))
    return (b"\r\n" if crlf else b"\n").join(out)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the database and ~40 inputs in command-line order: (path, bytes the scan sees or None for the missing one)"""
    import matchy_amd as M
    d = tmp_path_factory.mktemp("pack")
    b = M.DatabaseBuilder(build_epoch=1)
    for key, data in (("10.1.2.0/24", {"k": "net"}), ("192.0.2.7", {"k": "host"}), ("evil.example.com", {"k": "dom"}), ("*.bad.example.org", {"k": "glob"})):
        b.add_entry(key, data)
    dbp = d / "t.mxy"
    b.save(str(dbp))
    b.close()
    files = []
    for i in range(40):
        name, seen = f"host{i:02d}.log", None
        if i == 7:
            data = seen = b""                                               # empty
        elif i == 13:
            data = seen = _lines(i, 130) + b"\n"                            # above the limit: read the old way
            assert len(data) > BATCH // 4
        elif i == 20:
            name, seen = "rotated.log.gz", _lines(i, 30) + b"\n"            # a .gz in the middle
            data = gzip.compress(seen)
        elif i == 26:
            data = None                                                     # a path that does not exist
        elif i % 6 == 1:
            data = seen = _lines(i, 12 + i, crlf=True) + (b"\r\n" if i % 12 == 1 else b"")   # CRLF throughout, with and without a final one
        elif i % 3 == 0:
            data = seen = _lines(i, 10 + i)                                 # no final newline
        elif i == 38:
            data = seen = b"10.1.2.3"                                       # one hit, no newline at all
        else:
            data = seen = _lines(i, 8 + 2 * i) + b"\n"
        path = d / name
        if data is not None:
            path.write_bytes(data)
            assert name.endswith(".gz") or i == 13 or len(data) <= BATCH // 4, (i, len(data))
        files.append((path, seen))
    return dbp, files


def _run(cli, dbp, files, *flags):
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p, _ in files] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600)


COUNTS = [rb"\[INFO\] Files processed: ([\d,]+)", rb"\[INFO\] Files failed: ([\d,]+)", rb"\[INFO\] Lines processed: ([\d,]+)", rb"\[INFO\] Lines with matches: ([\d,]+) ",
          rb"\[INFO\] Total matches: ([\d,]+)", rb"\[INFO\] Candidates tested: ([\d,]+)"]


def _counts(stderr):
    out = []
    for pat in COUNTS:
        m = re.search(pat, stderr)
        assert m, (pat, stderr[-3000:])
        out.append(int(m.group(1).replace(b",", b"")))
    return out


@pytest.mark.parametrize("flags", [(), ("--line-numbers", "--input-line"), ("--tally=0",), ("--devices", "0,0"), ("--devices", "0,0", "--line-numbers")],
                         ids=["json", "line_numbers_input_line", "tally", "two_scanners", "two_scanners_line_numbers"])
def test_stdout_is_byte_identical(cli, corpus, flags):
    dbp, files = corpus
    plain = _run(cli, dbp, files, *flags)
    packed = _run(cli, dbp, files, *flags, "--pack-inputs")
    assert plain.returncode == packed.returncode == 1   # the missing path
    assert plain.stdout.count(b"\n") > 400
    assert packed.stdout == plain.stdout
    missing = str(files[26][0]).encode()
    assert plain.stderr.count(b"[ERROR] Failed to process " + missing) == packed.stderr.count(b"[ERROR] Failed to process " + missing) == 1


@pytest.mark.parametrize("flags", [(), ("--line-numbers",)], ids=["host_count", "line_context"])
def test_summary_counts_are_equal(cli, corpus, flags):
    dbp, files = corpus
    plain = _run(cli, dbp, files, "--format", "summary", "-s", *flags)
    packed = _run(cli, dbp, files, "--format", "summary", "-s", "--pack-inputs", *flags)
    assert plain.returncode == packed.returncode == 1
    assert plain.stdout == packed.stdout == b""
    want = _counts(plain.stderr)
    assert _counts(packed.stderr) == want
    total_lines = sum(seen.count(b"\n") for _, seen in files if seen is not None)
    assert want[0] == 39 and want[1] == 1 and want[2] == total_lines and want[3] > 150 and want[4] > 400
    assert b"Packed" not in plain.stderr
    m = re.search(rb"\[INFO\] Packed (\d+) inputs into (\d+) batches \((\d+) bytes of input in all\)", packed.stderr)
    assert m, packed.stderr[-3000:]
    n, batches, nbytes = (int(x) for x in m.groups())
    assert 1 < batches < n and n == 36                               # all but the empty, the large, the .gz and the missing one
    assert nbytes == sum(len(seen) for _, seen in files if seen is not None)   # the newlines the packer appended are not input


def test_all_good_inputs_exit_zero_and_few_files(cli, corpus):
    dbp, files = corpus
    good = [f for f in files if f[1] is not None]
    for subset in (good, good[:1], good[:2], [good[7]]):
        plain = _run(cli, dbp, subset)
        packed = _run(cli, dbp, subset, "--pack-inputs")
        assert plain.returncode == packed.returncode == 0, packed.stderr[-2000:]
        assert packed.stdout == plain.stdout


def test_pack_inputs_with_follow_is_refused(cli, corpus):
    dbp, files = corpus
    r = subprocess.run([cli, "match", str(dbp), str(files[0][0]), "--pack-inputs", "--follow"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--pack-inputs is not supported with --follow" in r.stderr and r.stdout == b""
