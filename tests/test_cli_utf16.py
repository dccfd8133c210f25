"""GPU: `matchy match --encoding=utf-16le|utf-16be|auto`. A UTF-16 input is transcoded on the GPU in front of the scan, so the command
prints on stdout exactly what it prints for the UTF-8 rendition of the same file under the same path: the two renditions live in two
directories and every run has its directory as cwd."""
import gzip
import subprocess
from pathlib import Path

import pytest

import gz_cases as G
import utf16_cases as U

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 4096
INDICATORS = ["10.1.2.5", "10.1.2.77", "192.0.2.7", "198.51.100.9", "evil.example.com", "cdn3.bad.example.org", G.MD5, "203.0.113.4", "www.example.net"]
FLAG_SETS = [("--format", "json"), ("--line-numbers", "--input-line"), ("--format", "summary", "--tally=5"), ("--gather-lines",), ("--render-on-gpu",)]
BOM = {"utf-16-le": b"\xff\xfe", "utf-16-be": b"\xfe\xff"}
FLAG = {"utf-16-le": "--encoding=utf-16le", "utf-16-be": "--encoding=utf-16be"}


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """dirs["utf-8"] and dirs[(codec, bom)] hold lf.log and crlf.log, the same text in each rendition; the database lies beside them"""
    d = tmp_path_factory.mktemp("cli_utf16")
    dbp = d / "t.mxy"
    dbp.write_bytes(G.blob())
    texts = {"lf.log": U.log_text(700, seed=21, indicators=INDICATORS), "crlf.log": U.log_text(500, seed=22, crlf=True, indicators=INDICATORS)}
    dirs = {}
    for key in ["utf-8"] + [(c, b) for c in BOM for b in (False, True)]:
        sub = d / ("utf8" if key == "utf-8" else f"{key[0]}{'-bom' if key[1] else ''}")
        sub.mkdir()
        for name, text in texts.items():
            (sub / name).write_bytes(text.encode("utf-8") if key == "utf-8" else (BOM[key[0]] if key[1] else b"") + text.encode(key[0]))
        dirs[key] = sub
    return dbp, dirs, texts


def run(cli, dbp, cwd, inputs, *flags, stdin=None):
    return subprocess.run([cli, "match", str(dbp)] + list(inputs) + ["--batch-bytes", str(BATCH)] + list(flags), capture_output=True, timeout=300, cwd=str(cwd), input=stdin)


_expected = {}


def expected(cli, dbp, dirs, name, flags):
    """stdout of the run on the UTF-8 rendition, once per (file, flags)"""
    if (name, flags) not in _expected:
        r = run(cli, dbp, dirs["utf-8"], [name], *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count(b"\n") >= (5 if "--tally=5" in flags else 100)
        _expected[name, flags] = r.stdout
    return _expected[name, flags]


@pytest.mark.parametrize("name", ["lf.log", "crlf.log"])
@pytest.mark.parametrize("bom", [False, True], ids=["nobom", "bom"])
@pytest.mark.parametrize("codec", ["utf-16-le", "utf-16-be"])
def test_same_output_as_the_utf8_rendition(cli, corpus, codec, bom, name):
    """LE and BE, with and without BOM, LF and CRLF, the input cut into many batches: every flag set prints what the UTF-8 file prints"""
    dbp, dirs, texts = corpus
    assert len(texts[name].encode(codec)) > 10 * BATCH
    for flags in FLAG_SETS:
        r = run(cli, dbp, dirs[codec, bom], [name], FLAG[codec], "-s", *flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == expected(cli, dbp, dirs, name, flags), flags
        info = [ln for ln in r.stderr.splitlines() if ln.startswith(b"[INFO] UTF-16:")]
        assert len(info) == 1 and b"1 inputs transcoded" in info[0] and b" 0 U+FFFD" in info[0], r.stderr[-2000:]
        assert f"({len(texts[name].encode('utf-16-le')) // 2} code units".encode() in info[0], info   # a pair counts as two


def test_auto_with_a_mix_of_inputs(cli, corpus, tmp_path):
    """auto decides per input: UTF-8 as bytes, FF FE little-endian, FE FF big-endian; the BOM is not part of the text"""
    dbp, dirs, texts = corpus
    a, b = tmp_path / "mixed", tmp_path / "plain"
    a.mkdir(); b.mkdir()
    parts = [("a.log", texts["lf.log"], None), ("b.log", texts["crlf.log"], "utf-16-le"), ("c.log", texts["lf.log"][:20000], "utf-16-be")]
    for name, text, codec in parts:
        (a / name).write_bytes(text.encode("utf-8") if codec is None else BOM[codec] + text.encode(codec))
        (b / name).write_bytes(text.encode("utf-8"))
    names = [p[0] for p in parts]
    for flags in FLAG_SETS:
        want = run(cli, dbp, b, names, *flags)
        got = run(cli, dbp, a, names, "--encoding=auto", "-s", *flags)
        assert want.returncode == got.returncode == 0, got.stderr[-2000:]
        assert got.stdout == want.stdout and want.stdout.count(b"\n") >= 5, flags
        assert b"[INFO] UTF-16: 2 inputs transcoded" in got.stderr
    # the same through several scanners on one device
    want = run(cli, dbp, b, names, "--line-numbers")
    got = run(cli, dbp, a, names, "--encoding=auto", "--line-numbers", "--devices", "0,0,0")
    assert got.returncode == 0 and got.stdout == want.stdout


def test_auto_leaves_a_file_without_bom_alone(cli, corpus):
    """auto on a UTF-16 file without a BOM is today's output: no records, no error, and no line about UTF-16"""
    dbp, dirs, _ = corpus
    today = run(cli, dbp, dirs["utf-16-le", False], ["lf.log"], "-s")
    auto = run(cli, dbp, dirs["utf-16-le", False], ["lf.log"], "--encoding=auto", "-s")
    assert today.returncode == auto.returncode == 0
    assert today.stdout == auto.stdout == b""
    assert b"UTF-16" not in auto.stderr and b"[INFO] Total matches: 0" in auto.stderr


def test_streams(cli, corpus, tmp_path):
    """stdin and a .gz input are read, not mapped: the first two bytes are looked at before the batch reader sees the stream"""
    dbp, dirs, texts = corpus
    text = texts["crlf.log"]
    for codec in BOM:
        for bom in (False, True):
            data = (BOM[codec] if bom else b"") + text.encode(codec)
            want = run(cli, dbp, tmp_path, ["-"], "--line-numbers", stdin=text.encode("utf-8"))
            for flag in (FLAG[codec],) + (("--encoding=auto",) if bom else ()):
                got = run(cli, dbp, tmp_path, ["-"], flag, "--line-numbers", stdin=data)
                assert got.returncode == want.returncode == 0, got.stderr[-2000:]
                assert got.stdout == want.stdout and want.stdout.count(b"\n") > 100
    a, b = tmp_path / "z16", tmp_path / "z8"
    a.mkdir(); b.mkdir()
    (a / "r.log.gz").write_bytes(gzip.compress(BOM["utf-16-be"] + text.encode("utf-16-be")))
    (b / "r.log.gz").write_bytes(gzip.compress(text.encode("utf-8")))
    want = run(cli, dbp, b, ["r.log.gz"])
    got = run(cli, dbp, a, ["r.log.gz"], "--encoding=auto")
    assert got.returncode == 0 and got.stdout == want.stdout and want.stdout.count(b"\n") > 100
    # an odd last byte and an unpaired surrogate: U+FFFD in the text, counted in the report
    odd = "src=10.1.2.5 ok\n".encode("utf-16-le") + b"\x00\xd8" + " evil.example.com ".encode("utf-16-le") + b"\x41"
    got = run(cli, dbp, tmp_path, ["-"], "--encoding=utf-16le", "-s", "--input-line", stdin=odd)
    assert got.returncode == 0 and got.stdout.count(b"\n") == 2 and b"evil.example.com" in got.stdout, got.stderr[-2000:]
    assert b" 2 U+FFFD written" in got.stderr


@pytest.mark.parametrize("flags,message", [
    (("--follow",), "--encoding is not supported with --follow"),
    (("--pack-inputs",), "--encoding is not supported with --pack-inputs"),
    (("--gz-on-gpu",), "--encoding is not supported with --gz-on-gpu"),
    (("--gz-on-gpu", "--gz-members"), "--encoding is not supported with --gz-on-gpu"),
    (("--gz-members",), "--encoding is not supported with --gz-members"),
    (("--gz-windows",), "--encoding is not supported with --gz-windows"),
    (("--gz-stream-windows",), "--encoding is not supported with --gz-stream-windows"),
    (("--gz-pieces",), "--encoding is not supported with --gz-pieces"),
    (("--whole-lines",), "--encoding is not supported with --whole-lines"),
])
def test_refused_combinations(cli, corpus, flags, message):
    dbp, dirs, _ = corpus
    for enc in ("--encoding=utf-16le", "--encoding=auto"):
        r = run(cli, dbp, dirs["utf-8"], ["lf.log"], enc, *flags)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.decode().strip().splitlines()[-1].startswith("Error: " + message), r.stderr


def test_unknown_encoding(cli, corpus):
    dbp, dirs, _ = corpus
    r = run(cli, dbp, dirs["utf-8"], ["lf.log"], "--encoding=latin-1")
    assert r.returncode == 1 and b"Unknown encoding: latin-1" in r.stderr and r.stdout == b""
