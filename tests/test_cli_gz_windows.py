"""GPU: `matchy match --gz-on-gpu --gz-members --gz-windows` — multi-member .gz inputs LARGER than a batch go out as chains of windows of
whole members. The command prints the same records, in the same place, and counts the same as without any gz flag; a file whose chain
ends early (a corrupt member, a line longer than the carry bound) is finished by the host from the bytes its windows consumed."""
import gzip
import os
import re
import subprocess
from pathlib import Path

import pytest

import gz_cases as G
import gz_files_cases as F
import gz_window_cases as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 65536
MAX_MEMBER = BATCH // 4
MAX_CARRY = 2048
COUNTS = [rb"\[INFO\] Files processed: ([\d,]+)", rb"\[INFO\] Files failed: ([\d,]+)", rb"\[INFO\] Lines processed: ([\d,]+)", rb"\[INFO\] Lines with matches: ([\d,]+) ",
          rb"\[INFO\] Total matches: ([\d,]+)", rb"\[INFO\] Candidates tested: ([\d,]+)"]
WINDOWED = ("wbgzf", "mbig", "wcorrupt", "wlong")        # larger than a pack: chains of windows
ON_HOST = ("wcorrupt", "wlong")                           # of those, the chains that end early
FLAGS = ("--gz-on-gpu", "--gz-members", "--gz-windows")
MODES = [(), ("--line-numbers", "--input-line"), ("--gather-lines",), ("--render-on-gpu",), ("--render-on-gpu", "--line-numbers")]
MODE_IDS = ["json", "line_numbers_input_line", "gather_lines", "render_on_gpu", "render_on_gpu_line_numbers"]


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


def windows_of(data):
    return W.walk_windows(data, BATCH, BATCH - MAX_CARRY, MAX_MEMBER)


def window_texts(data, windows):
    out, at = [], 0
    for end, _, _, _ in windows:
        out.append(gzip.decompress(data[at:end]))
        at = end
    return out


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """the database and the inputs in command-line order: [(path, kind)]; plain files and small .gz files around four large ones"""
    d = tmp_path_factory.mktemp("gzw")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    files = []

    def put(name, kind, data):
        (d / name).write_bytes(data)
        files.append((d / name, kind))
    for i in range(12):
        text = G.log(5 + 2 * i, seed=40 + i, final_newline=i % 4 != 0)
        if i % 5 == 0:
            put(f"plain{i:02d}.log", "plain", text)
        else:
            put(f"rot{i:02d}.log.gz", "gz", gzip.compress(text, 1 + i % 9))
        if i == 2:      # BGZF-style, about six batches of text, cut mid-line, the empty block last
            text = G.log(4000, seed=500, final_newline=False)
            assert 5 * BATCH < len(text) < 8 * BATCH
            data = F.bgzf_file(text, 3001)
            ws, stop = windows_of(data)
            assert stop == len(data) and len(ws) >= 6
            put("wbgzf.log.gz", "wbgzf", data)
        elif i == 4:    # seven members, more text than a pack holds
            data = b"".join(F.member(G.log(80, seed=330 + k)) for k in range(7))
            ws, stop = windows_of(data)
            assert len(gzip.decompress(data)) > BATCH and stop == len(data) and len(ws) == 2
            put("mbig.log.gz", "mbig", data)
        elif i == 7:    # the corrupt member (a flipped CRC bit) lies in the third window; two more windows would follow
            parts = [bytearray(F.member(G.log(60, seed=600 + k, final_newline=k % 3 != 0))) for k in range(45)]
            good = b"".join(bytes(p) for p in parts)
            ws, stop = windows_of(good)
            assert stop == len(good) and len(ws) >= 4
            third = ws[2][3]                                   # where the members of the third window start
            k = F.split_members(good).index(third[len(third) // 2])
            parts[k][-6] ^= 0x10
            data = b"".join(bytes(p) for p in parts)
            assert windows_of(data) == (ws, stop)              # the walk does not see the flip
            put("wcorrupt.log.gz", "wcorrupt", data)
        elif i == 9:    # one line longer than the carry bound, across the end of the first window
            head = G.log(600, seed=700)
            head = head[:head.rfind(b"\n", 0, 57000) + 1]
            long_line = b"GET /long from " + F.NEEDLE + b" " + b"x" * (MAX_CARRY + 3000) + b" done\n"
            text = head + long_line + G.log(900, seed=701)
            data = b"".join(F.member(text[at:at + 6000]) for at in range(0, len(text), 6000))
            ws, stop = windows_of(data)
            assert stop == len(data) and len(ws) >= 2
            model = W.chain(window_texts(data, ws), MAX_CARRY)
            assert len(model) == 1 and model[0][5] == 1          # NO_LINE_END in the first window: the host reads the whole file
            put("wlong.log.gz", "wlong", data)
    return dbp, files


def _run(cli, dbp, files, *flags):
    env = dict(os.environ, MATCHY_AMD_GZ_MAX_CARRY=str(MAX_CARRY))
    return subprocess.run([cli, "match", str(dbp)] + [str(p) for p, _ in files] + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=600, env=env)


def _counts(stderr, failed=True):
    out = []
    for pat in COUNTS if failed else COUNTS[:1] + COUNTS[2:]:
        m = re.search(pat, stderr)
        assert m, (pat, stderr[-3000:])
        out.append(int(m.group(1).replace(b",", b"")))
    return out


def _errors(r):
    return [ln for ln in r.stderr.splitlines() if ln.startswith(b"[ERROR]")]


def _of(stdout, files, kind):
    names = [str(p).encode() for p, k in files if k == kind]
    return [ln for ln in stdout.splitlines() if any(n in ln for n in names)]


def _expected_windows(files):
    """windows the GPU accepts: every window of the good chains, the two in front of the corrupt member, none of the long line's file"""
    n = 0
    for p, k in files:
        if k in ("wbgzf", "mbig"):
            n += len(windows_of(p.read_bytes())[0])
    return n + 2


@pytest.mark.parametrize("flags", MODES, ids=MODE_IDS)
def test_same_stdout_with_and_without_the_flags(cli, corpus, flags):
    """stdout is byte-identical to the run without gz flags, and the [ERROR] lines are the same"""
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", *flags)
    new = _run(cli, dbp, files, "-s", *flags, *FLAGS)
    assert old.returncode == new.returncode == 1                # the corrupt file
    assert old.stdout.count(b"\n") > 3000
    assert _errors(old) == _errors(new) and len(_errors(old)) == 1
    for kind in WINDOWED:
        assert len(_of(old.stdout, files, kind)) > 100, kind
    if old.stdout != new.stdout:                                # name the input instead of printing megabytes
        bad = [k for _, k in files if _of(old.stdout, files, k) != _of(new.stdout, files, k)]
        raise AssertionError(f"stdout differs, in the records of {sorted(set(bad))} ({len(old.stdout)} and {len(new.stdout)} bytes)")


def test_a_chain_that_got_further_than_the_host_reports_the_lines_in_between(cli, corpus, tmp_path):
    """The limit of the fallback, held as it is documented (Windows). When the decoder fails, the run without gz flags
    loses the batch it was filling: it reports the text up to its last batch cut, which lies less than one batch in front of the
    failure. The windows report the text up to the failed window's start, which does so too. Where the host's cut is the later one
    (wcorrupt.log.gz above) the host's second pass reports what lies between and stdout is identical; where the windows got further —
    here: the corrupt member is the FIRST of the third window — the windowed run has already reported the verified complete lines in
    between. They are not taken back: its records are those of the plain run, then those lines, nothing else; [ERROR] and exit status
    are the same."""
    dbp, files = corpus
    src = [p for p, k in files if k == "wcorrupt"][0].read_bytes()
    cuts = F.split_members(src)
    parts = [bytearray(src[a:e]) for a, e in zip(cuts, cuts[1:] + [len(src)])]
    ws, stop = windows_of(src)
    k_old = [k for k in range(len(parts)) if not _member_ok(bytes(parts[k]))]
    assert len(k_old) == 1
    parts[k_old[0]][-6] ^= 0x10                                 # heal the member of the corpus file
    k_new = cuts.index(ws[2][3][0])                             # the first member of the third window
    parts[k_new][-6] ^= 0x10
    data = b"".join(bytes(p) for p in parts)
    assert windows_of(data) == (ws, stop) and not _member_ok(bytes(parts[k_new])) and all(_member_ok(bytes(p)) for k, p in enumerate(parts) if k != k_new)
    path = tmp_path / "wearly.log.gz"
    path.write_bytes(data)
    mine = [(files[0][0], "plain"), (path, "wearly"), (files[1][0], "gz")]
    old = _run(cli, dbp, mine, "-s", "--line-numbers")
    new = _run(cli, dbp, mine, "-s", "--line-numbers", *FLAGS)
    # zlib names the file by its descriptor ("<fd:5>"), whose number depends on what else the process has open at that moment
    fd = lambda r: [re.sub(rb"<fd:\d+>", b"<fd>", ln) for ln in _errors(r)]   # noqa: E731
    assert old.returncode == new.returncode == 1 and fd(old) == fd(new) and len(fd(old)) == 1
    a, b = _of(old.stdout, mine, "wearly"), _of(new.stdout, mine, "wearly")
    rest = lambda r: [ln for ln in r.stdout.splitlines() if path.name.encode() not in ln]   # noqa: E731
    assert rest(old) == rest(new) and len(rest(old)) > 5
    good_text = gzip.decompress(data[:ws[1][0]])                 # the members of the first two windows
    consumed = good_text.rfind(b"\n") + 1                       # what the two windows report: their complete lines
    want = subprocess.run([cli, "match", str(dbp), "-", "--batch-bytes", str(BATCH), "--line-numbers"], input=good_text[:consumed], capture_output=True, timeout=600)
    assert want.returncode == 0
    assert [ln.replace(str(path).encode(), b"stdin") for ln in b] == want.stdout.splitlines()
    assert b[:len(a)] == a and 100 < len(a) < len(b)
    lines = new.stdout.splitlines()
    at = lines.index(b[0])
    assert lines[at:at + len(b)] == b                            # one block, at the file's place on the command line
    print(f"wearly: {len(a)} records without the flags, {len(b)} with them; the windows consumed {consumed} bytes of text")


def _member_ok(m):
    try:
        gzip.decompress(m)
        return True
    except Exception:
        return False


def test_summary_counts_and_tally(cli, corpus):
    """--format summary -s counts and --tally are equal"""
    dbp, files = corpus
    old = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0")
    new = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0", *FLAGS)
    assert old.returncode == new.returncode == 1
    assert _counts(old.stderr) == _counts(new.stderr) and _counts(old.stderr)[4] > 3000
    assert old.stdout == new.stdout and old.stdout.count(b"\n") > 10


def test_summary_counts_and_tally_without_the_corrupt_input(cli, corpus):
    dbp, files = corpus
    files = [(p, k) for p, k in files if k != "wcorrupt"]
    old = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0")
    new = _run(cli, dbp, files, "-s", "--format", "summary", "--tally=0", *FLAGS)
    assert old.returncode == new.returncode == 0
    assert _counts(old.stderr, failed=False) == _counts(new.stderr, failed=False) and _counts(old.stderr, failed=False)[3] > 2500
    assert old.stdout == new.stdout and old.stdout.count(b"\n") > 10
    m = re.search(rb"\[INFO\] gz windows on the GPU: (\d+) windows of (\d+) files, (\d+) finished on the host\n", new.stderr)
    assert m and tuple(map(int, m.groups())) == (_expected_windows(files) - 2, 3, 1), new.stderr[-2000:]


def test_statistics(cli, corpus):
    """-s reports the windows, the windowed files and those finished on the host; without --gz-windows the statistics are what they
    were: the large files are read on the host and no window line is printed"""
    dbp, files = corpus
    small = sum(1 for _, k in files if k == "gz")
    new = _run(cli, dbp, files, "-s", *FLAGS)
    m = re.search(rb"\[INFO\] gz windows on the GPU: (\d+) windows of (\d+) files, (\d+) finished on the host\n", new.stderr)
    assert m, new.stderr[-3000:]
    n_windows, n_files, n_host = map(int, m.groups())
    assert (n_files, n_host) == (len(WINDOWED), len(ON_HOST)) and n_files >= 2 and n_host >= 2
    assert n_windows == _expected_windows(files) >= 10
    inflated = rb"\[INFO\] Inflated (\d+) \.gz inputs on the GPU in (\d+) batches \((\d+) -> (\d+) bytes\), (\d+) read on the host\n"
    with_windows = re.search(inflated, new.stderr)
    old = _run(cli, dbp, files, "-s", "--gz-on-gpu", "--gz-members")
    without = re.search(inflated, old.stderr)
    assert without and with_windows and without.groups() == with_windows.groups()
    assert (int(without.group(1)), int(without.group(5))) == (small, 0)      # the large files are not tried: they are on the host
    assert b"gz windows" not in old.stderr
    assert old.stdout == _run(cli, dbp, files).stdout and old.returncode == 1


def test_refusals(cli, corpus):
    dbp, files = corpus
    one = str(files[1][0])
    for flags in (("--gz-windows",), ("--gz-windows", "--gz-on-gpu"), ("--gz-windows", "--gz-members"), ("--gz-windows", "--whole-lines")):
        r = subprocess.run([cli, "match", str(dbp), one, *flags], capture_output=True, timeout=60)
        assert r.returncode == 1 and b"--gz-windows needs --gz-on-gpu --gz-members" in r.stderr and not r.stdout, flags
    r = subprocess.run([cli, "match", str(dbp), one, *FLAGS, "--whole-lines"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"--whole-lines is not supported with --gz-on-gpu" in r.stderr
    r = subprocess.run([cli, "match", str(dbp), one, *FLAGS, "--follow"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"not supported with --follow" in r.stderr
