"""GPU: `matchy match --whole-lines` — every input line is one query and the records are the ordinary match records, checked against
the model of tests/whole_lines_cases.py (oracle + the library's host path per line), rendered the way the host NDJSON writer lays a
record out (sorted keys; cidr / data / prefix_len for an address, data / pattern_count for a string)."""
import gzip
import json
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tally_cases as T         # noqa: E402
import whole_lines_cases as W   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = W.ROOT
CLI = ROOT / "matchy_amd" / "bin" / "matchy"


def expected_records(recs, buf, source, lines=False):
    """the model's records as the objects the NDJSON writer prints for them"""
    ends = [i for i, b in enumerate(buf) if b == 0x0A] + [len(buf)]
    out = []
    for w in recs:
        text = buf[w["start"]:w["end"]].decode()
        if w["kind"] == "ip":
            o = {"cidr": w["cidr"], "data": w["data"][0], "match_type": "ip", "matched_text": text, "prefix_len": w["prefix_len"]}
        else:
            o = {"match_type": "pattern", "matched_text": text, "pattern_count": len(w["ids"])}
            if w["data"]:
                o["data"] = w["data"]
        if lines:
            o["line_number"] = w["line"] + 1
            o["input_line"] = buf[w["start"]:ends[w["line"]]].decode()   # the line as it stands: a '\r' in front of the '\n' belongs to it
        o["source"] = source
        o["timestamp"] = "0.000"
        out.append(o)
    return out


@pytest.fixture(scope="module")
def setup(oracle, tmp_path_factory):
    import matchy_amd as M
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    d = tmp_path_factory.mktemp("cli_whole_lines")
    blob = W.build_blob(W.rule_entries())
    (d / "db.mxy").write_bytes(blob)
    files = {"rules": W.rule_list(), "repeats": W.repeats_list()}
    db = M.Database(blob)
    odb = W.Memo(oracle.Database(blob))
    host = W.memoized(W.host_from_db(db))
    out = {"db": str(d / "db.mxy"), "dir": d}
    for name, buf in files.items():
        (d / (name + ".txt")).write_bytes(buf)
        recs, ctr = W.model(odb, host, buf)
        out[name] = {"path": str(d / (name + ".txt")), "buf": buf, "recs": recs, "ctr": ctr}
    (d / "rules.txt.gz").write_bytes(gzip.compress(files["rules"]))
    odb.close()
    db.close()
    return out


def _run(args, stdin=None):
    return subprocess.run([str(CLI)] + args, input=stdin, capture_output=True, timeout=600)


def _objects(stdout):
    lines = stdout.decode().splitlines()
    objs = [json.loads(ln) for ln in lines]
    for ln, o in zip(lines, objs):
        assert list(o) == sorted(o), ln   # the writer's key order
    return objs


def test_two_files_stdin_and_gz_give_the_models_records(setup):
    a, b = setup["rules"], setup["repeats"]
    p = _run(["match", setup["db"], a["path"], b["path"], "--whole-lines", "-s"])
    assert p.returncode == 0, p.stderr[-2000:]
    want = expected_records(a["recs"], a["buf"], a["path"]) + expected_records(b["recs"], b["buf"], b["path"])
    assert _objects(p.stdout) == want
    err = p.stderr.decode().replace(",", "")
    tot = {k: a["ctr"][k] + b["ctr"][k] for k in a["ctr"]}
    assert "[INFO] Whole-line queries: %d (%d addresses %d strings %d not valid UTF-8)" % (tot["queries"], tot["address"], tot["string"], tot["invalid_utf8"]) in err, err[-1500:]
    assert "[INFO] Total matches: %d" % len(want) in err
    # standard input, and a .gz through the host reader
    p = _run(["match", setup["db"], "-", "--whole-lines"], stdin=a["buf"])
    assert p.returncode == 0, p.stderr[-2000:]
    got = _objects(p.stdout)
    src = got[0]["source"]
    assert got == expected_records(a["recs"], a["buf"], src)
    gz = str(setup["dir"] / "rules.txt.gz")
    p = _run(["match", setup["db"], gz, "--whole-lines"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert _objects(p.stdout) == expected_records(a["recs"], a["buf"], gz)
    # without the flag the list is log text: other records
    plain = _run(["match", setup["db"], a["path"]])
    assert plain.returncode == 0 and plain.stdout != _run(["match", setup["db"], a["path"], "--whole-lines"]).stdout


def test_line_numbers_and_input_line(setup):
    b = setup["repeats"]
    p = _run(["match", setup["db"], b["path"], "--whole-lines", "--line-numbers", "--input-line"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert _objects(p.stdout) == expected_records(b["recs"], b["buf"], b["path"], lines=True)


def test_summary_with_tally(setup):
    b = setup["repeats"]
    want = T.ordered(W.model_tally(b["recs"], b["buf"]))
    p = _run(["match", setup["db"], b["path"], "--whole-lines", "--format", "summary", "--tally=5", "-s"])
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [json.loads(ln) for ln in p.stdout.decode().splitlines()]
    assert [(r["matched_text"].encode(), r["item_type"], r["count"]) for r in rows] == want[:5] and len(want) > 5
    assert "[INFO] Distinct matched values: %d" % len(want) in p.stderr.decode()


def test_two_scanners_on_one_device(setup):
    a, b = setup["rules"], setup["repeats"]
    p = _run(["match", setup["db"], a["path"], b["path"], "--whole-lines", "--devices", "0,0", "--batch-bytes", "4096"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert _objects(p.stdout) == expected_records(a["recs"], a["buf"], a["path"]) + expected_records(b["recs"], b["buf"], b["path"])


@pytest.mark.parametrize("flag", ["--extractors=ipv4", "--pack-inputs", "--gz-on-gpu", "--gather-lines", "--render-on-gpu"])
def test_refused_flag_pairs(setup, flag):
    p = _run(["match", setup["db"], setup["rules"]["path"], "--whole-lines", flag])
    assert p.returncode != 0 and p.stdout == b""
    assert "--whole-lines is not supported with " + flag.split("=")[0] in p.stderr.decode()


def test_help_names_the_flag():
    p = _run(["match"])
    assert "--whole-lines" in p.stderr.decode()
