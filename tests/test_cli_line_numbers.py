"""GPU: `matchy match --line-numbers --input-line` — "line_number" (1-based per input) and "input_line" in every record, from the line
context the scan computes on the device; without the flags the command prints what it always printed (the CPU oracle's lines)."""
import json
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
INDICATORS = [b"10.1.2.3", b"192.0.2.7", b"evil.example.com", b"bad.example.org"]


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    return str(CLI)


def _inputs():
    a, b = [], []
    for i in range(420):
        if i % 7 == 3:
            a.append(b"GET /p%d from 10.1.2.3 to evil.example.com status ok" % i)          # two hits in one line
        elif i % 11 == 5:
            a.append(b"caf\xc3\xa9 192.0.2.7 \xe2\x82\xac ok\r")                              # valid multi-byte text, '\r' stays in the line
        elif i == 200:
            a.append(b"broken \xff byte \xe2\x82 bad.example.org \xf0\x9f tail")             # ill-formed UTF-8 in a matching line
        elif i % 5 == 0:
            a.append(b"")
        else:
            a.append(b"nothing to see in line %d of this input, only filler text" % i)
    for i in range(300):
        b.append(b"second input line %d 10.1.2.3" % i if i % 13 == 0 else b"second input filler %d ..............................." % i)
    b.append(b"last line without a newline bad.example.org")
    return b"\n".join(a) + b"\n", b"\n".join(b)


def _model(data):
    """[(line_number, matched_text)] in file order, lines with matches"""
    pat = re.compile(b"|".join(re.escape(x) for x in INDICATORS))
    out, lines = [], data.split(b"\n")
    for n, line in enumerate(lines, 1):
        out += [(n, m.group().decode()) for m in pat.finditer(line)]
    return out, lines, len({n for n, _ in out})


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, timeout=600, **kw)


def _check(records, data, source=None):
    want, lines, _ = _model(data)
    assert [(r["line_number"], r["matched_text"]) for r in records] == want
    for r in records:
        assert list(r) == sorted(r)
        assert r["input_line"] == lines[r["line_number"] - 1].decode("utf-8", "replace")
        if source is not None:
            assert r["source"] == source


def test_line_numbers_and_input_lines(cli, tmp_path, oracle):
    import matchy_amd as M
    b = M.DatabaseBuilder(build_epoch=1)
    b.add_entry("10.1.2.0/24", {"k": "net"})
    b.add_entry("192.0.2.7", {"k": "host"})
    b.add_entry("evil.example.com", {"k": "dom"})
    b.add_entry("bad.example.org", {"k": "dom2"})
    dbp = tmp_path / "t.mxy"
    b.save(str(dbp))
    b.close()
    d1, d2 = _inputs()
    p1, p2 = tmp_path / "one.log", tmp_path / "two.log"
    p1.write_bytes(d1)
    p2.write_bytes(d2)
    assert len(d1) > 3 * 4096 and len(d2) > 3 * 4096   # several batches per input
    r = _run([cli, "match", str(dbp), str(p1), str(p2), "--line-numbers", "--input-line", "--batch-bytes", "4096", "-s"])
    assert r.returncode == 0, r.stderr
    recs = [json.loads(l) for l in r.stdout.decode("utf-8").splitlines()]
    n1 = len(_model(d1)[0])
    assert n1 > 60 and len(recs) == n1 + len(_model(d2)[0])
    _check(recs[:n1], d1, str(p1))
    _check(recs[n1:], d2, str(p2))   # the count starts again with every input
    assert any("�" in x["input_line"] for x in recs) and recs[-1]["line_number"] == 301
    lwm = _model(d1)[2] + _model(d2)[2]
    assert f"[INFO] Lines with matches: {lwm:,} ".encode() in r.stderr, r.stderr
    # one flag alone
    r = _run([cli, "match", str(dbp), str(p1), "--line-numbers", "--batch-bytes", "4096"])
    only = [json.loads(l) for l in r.stdout.decode().splitlines()]
    assert r.returncode == 0 and all("input_line" not in x and list(x) == sorted(x) for x in only)
    assert [(x["line_number"], x["matched_text"]) for x in only] == _model(d1)[0]
    r = _run([cli, "match", str(dbp), str(p2), "--input-line", "--batch-bytes", "4096"])
    assert r.returncode == 0
    _check([json.loads(l) for l in r.stdout.decode().splitlines()], d2, str(p2))
    # stdin, and two scanners on one device: the printer numbers the batches in sequence order whatever worker scanned them
    r = _run([cli, "match", str(dbp), "-", "--line-numbers", "--input-line", "--batch-bytes", "4096"], input=d1)
    assert r.returncode == 0, r.stderr
    _check([json.loads(l) for l in r.stdout.decode().splitlines()], d1, "stdin")
    r = _run([cli, "match", str(dbp), str(p1), str(p2), "--line-numbers", "--input-line", "--batch-bytes", "4096", "--devices", "0,0", "-s"])
    assert r.returncode == 0, r.stderr
    recs2 = [json.loads(l) for l in r.stdout.decode().splitlines()]
    assert recs2 == recs and f"[INFO] Lines with matches: {lwm:,} ".encode() in r.stderr
    # without the flags: the lines the CPU oracle renders, and the same count from the host-side loop
    odb = oracle.Database(dbp.read_bytes())
    want = odb.scan(d1, source=str(p1))[1] + odb.scan(d2, source=str(p2))[1]
    r = _run([cli, "match", str(dbp), str(p1), str(p2), "--batch-bytes", "4096", "-s"])
    assert r.returncode == 0 and r.stdout.decode().splitlines() == want
    assert f"[INFO] Lines with matches: {lwm:,} ".encode() in r.stderr
    assert [{k: v for k, v in x.items() if k not in ("line_number", "input_line")} for x in recs] == [json.loads(l) for l in want]
