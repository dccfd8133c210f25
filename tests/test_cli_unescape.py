"""GPU: `matchy match --unescape=percent|json|json+percent`. The batches of an input are decoded on the GPU in front of the scan, so the
command prints on stdout exactly what it prints for the pre-decoded file (tests/unescape_cases.py's reference) under the same path: the
two renditions live in two directories and every run has its directory as cwd. An escape for a line end becomes a space, so the
pre-decoded file has the raw file's lines and the line numbers are the raw file's."""
import gzip
import json
import subprocess
from pathlib import Path

import pytest

import unescape_cases as U
from test_gpu_unescape import mixed_log

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 4096
FLAG_SETS = [("--format", "json"), ("--line-numbers", "--input-line"), ("--format", "summary", "--tally=5"), ("--gather-lines",), ("--render-on-gpu",),
             ("--render-on-gpu", "--line-numbers")]
MODES = {"percent": U.PERCENT, "json": U.JSON, "json+percent": U.PERCENT | U.JSON}
ISSUE_LINES = [
    b"GET /r?url=https%3A%2F%2Fevil.com%2Fpath&a=2001%3Adb8%3A%3A1 HTTP/1.1\n",
    b'{"msg":"{\\"host\\":\\"evil.com\\",\\"ip\\":\\"10.1.2.3\\"}"}\n',
    b'{"msg":"line1\\nevil.com\\tnext","u":"https:\\/\\/evil.com\\/x","e":"evil\\u002ecom"}\n',
]


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """raw/ and decoded/ hold app.log and issue.log, escaped and pre-decoded (json+percent); two databases lie beside them"""
    import gz_cases as G
    import matchy_amd as M
    d = tmp_path_factory.mktemp("cli_unescape")
    dbp, small = d / "t.mxy", d / "small.mxy"
    dbp.write_bytes(G.blob())
    b = M.DatabaseBuilder(build_epoch=1)
    for entry in ("evil.com", "10.1.2.3", "2001:db8::1"):
        b.add_entry(entry, {"k": entry})
    small.write_bytes(b.build())
    b.close()
    raw = {"app.log": b"".join(mixed_log(2500, seed=31)), "issue.log": b"".join(ISSUE_LINES)}
    assert len(raw["app.log"]) > 10 * BATCH
    dirs = {"raw": d / "raw", "decoded": d / "decoded"}
    for sub in dirs.values():
        sub.mkdir()
    for name, data in raw.items():
        (dirs["raw"] / name).write_bytes(data)
        (dirs["decoded"] / name).write_bytes(U.reference(data, U.PERCENT | U.JSON)[0])
    return dbp, small, dirs, raw


def run(cli, dbp, cwd, inputs, *flags, stdin=None):
    return subprocess.run([cli, "match", str(dbp)] + list(inputs) + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=300, cwd=str(cwd), input=stdin)


def records(out):
    return [json.loads(line) for line in out.splitlines()]


def test_the_lines_of_the_issue(cli, corpus):
    """each of the three lines gives no record as it is; decoded, they give the domain three times (and twice more on the third line),
    the IPv4 and the IPv6 address, on the raw file's line numbers"""
    _, small, dirs, _ = corpus
    today = run(cli, small, dirs["raw"], ["issue.log"], "--line-numbers")
    assert today.returncode == 0 and today.stdout == b"", today.stderr[-2000:]
    got = run(cli, small, dirs["raw"], ["issue.log"], "--unescape=json+percent", "--line-numbers", "--input-line", "-s")
    assert got.returncode == 0, got.stderr[-2000:]
    recs = records(got.stdout)
    found = sorted((r["line_number"], r["matched_text"]) for r in recs)
    assert found == [(1, "2001:db8::1"), (1, "evil.com"), (2, "10.1.2.3"), (2, "evil.com"), (3, "evil.com"), (3, "evil.com"), (3, "evil.com")], found
    assert {r["input_line"] for r in recs if r["line_number"] == 2} == {'{"msg":"{"host":"evil.com","ip":"10.1.2.3"}"}'}   # the decoded line
    info = [ln for ln in got.stderr.splitlines() if ln.startswith(b"[INFO] Unescape:")]
    assert len(info) == 1 and b"1 batches decoded" in info[0] and b" 0 U+FFFD written, 1 LF escapes as spaces" in info[0], got.stderr[-2000:]
    # one grammar alone decodes its own lines only
    pct = records(run(cli, small, dirs["raw"], ["issue.log"], "--unescape=percent", "--line-numbers").stdout)
    assert sorted((r["line_number"], r["matched_text"]) for r in pct) == [(1, "2001:db8::1"), (1, "evil.com")]
    js = records(run(cli, small, dirs["raw"], ["issue.log"], "--unescape=json", "--line-numbers").stdout)
    assert sorted({r["line_number"] for r in js}) == [2, 3] and len(js) == 5


def test_same_output_as_the_decoded_file(cli, corpus):
    """the input cut into many batches: every flag set prints what the pre-decoded file prints without the flag (the same path in
    another directory, so `source` is the same), and the raw file without the flag gives fewer records"""
    dbp, _, dirs, raw = corpus
    for flags in FLAG_SETS:
        want = run(cli, dbp, dirs["decoded"], ["app.log"], *flags)
        got = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=json+percent", "-s", *flags)
        assert want.returncode == got.returncode == 0, got.stderr[-2000:]
        assert got.stdout == want.stdout, flags
        assert want.stdout.count(b"\n") >= (5 if "--tally=5" in flags else 100)
        info = [ln for ln in got.stderr.splitlines() if ln.startswith(b"[INFO] Unescape:")]
        assert len(info) == 1 and f"({len(raw['app.log'])} -> {len(U.reference(raw['app.log'], 3)[0])} bytes".encode() in info[0], info
    plain = run(cli, dbp, dirs["raw"], ["app.log"])
    full = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=json+percent")
    assert plain.returncode == 0 and full.stdout.count(b"\n") >= plain.stdout.count(b"\n") + 3


def test_line_numbers_are_those_of_the_raw_file(cli, corpus):
    """every record's line number names a raw line that holds the indicator in some form: %0A and \\n did not shift the count"""
    dbp, _, dirs, raw = corpus
    got = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=json+percent", "--line-numbers", "--input-line")
    assert got.returncode == 0
    raw_lines = raw["app.log"].split(b"\n")
    recs = records(got.stdout)
    assert len(recs) > 100 and any(b"%0A" in raw_lines[r["line_number"] - 1] or b"\\n" in raw_lines[r["line_number"] - 1] for r in recs)
    for r in recs:
        line = raw_lines[r["line_number"] - 1]
        assert U.reference(line, 3)[0].decode("utf-8") == r["input_line"]
    # the same through several scanners on one device
    multi = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=json+percent", "--line-numbers", "--input-line", "--devices", "0,0,0")
    assert multi.returncode == 0 and multi.stdout == got.stdout


def test_streams(cli, corpus, tmp_path):
    """stdin and a host-inflated .gz input are read, not mapped"""
    dbp, _, dirs, raw = corpus
    data = raw["app.log"]
    decoded = (dirs["decoded"] / "app.log").read_bytes()
    want = run(cli, dbp, tmp_path, ["-"], "--line-numbers", stdin=decoded)
    got = run(cli, dbp, tmp_path, ["-"], "--unescape=json+percent", "--line-numbers", stdin=data)
    assert got.returncode == want.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want.stdout and want.stdout.count(b"\n") > 100
    a, b = tmp_path / "zraw", tmp_path / "zdec"
    a.mkdir(); b.mkdir()
    (a / "r.log.gz").write_bytes(gzip.compress(data))
    (b / "r.log.gz").write_bytes(gzip.compress(decoded))
    want = run(cli, dbp, b, ["r.log.gz"])
    got = run(cli, dbp, a, ["r.log.gz"], "--unescape=json+percent")
    assert got.returncode == 0 and got.stdout == want.stdout and want.stdout.count(b"\n") > 100


@pytest.mark.parametrize("flags,message", [
    (("--follow",), "--unescape is not supported with --follow"),
    (("--pack-inputs",), "--unescape is not supported with --pack-inputs"),
    (("--gz-on-gpu",), "--unescape is not supported with --gz-on-gpu"),
    (("--gz-on-gpu", "--gz-members"), "--unescape is not supported with --gz-on-gpu"),
    (("--gz-members",), "--unescape is not supported with --gz-members"),
    (("--gz-windows",), "--unescape is not supported with --gz-windows"),
    (("--gz-stream-windows",), "--unescape is not supported with --gz-stream-windows"),
    (("--gz-pieces",), "--unescape is not supported with --gz-pieces"),
    (("--whole-lines",), "--unescape is not supported with --whole-lines"),
    (("--encoding=utf-16le",), "--unescape is not supported with --encoding"),
])
def test_refused_combinations(cli, corpus, flags, message):
    dbp, _, dirs, _ = corpus
    for mode in MODES:
        r = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=" + mode, *flags)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().strip().splitlines()[-1].startswith("Error: " + message), r.stderr


def test_unknown_grammar(cli, corpus):
    dbp, _, dirs, _ = corpus
    r = run(cli, dbp, dirs["raw"], ["app.log"], "--unescape=html")
    assert r.returncode == 1 and b"Unknown escape grammar: html" in r.stderr and r.stdout == b""
