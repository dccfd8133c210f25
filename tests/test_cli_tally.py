"""GPU: `matchy match --tally[=N]` — behind the match records one JSON line per distinct matched value, the N most frequent, with the
value's database entry as `matchy query` prints it; checked against a Counter over the oracle's match set (tests/tally_cases.py)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tally_cases as T   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = T.ROOT
CLI = ROOT / "matchy_amd" / "bin" / "matchy"


@pytest.fixture(scope="module")
def setup(oracle, tmp_path_factory):
    import matchy_amd.build as B
    B.build()
    assert CLI.exists()
    d = tmp_path_factory.mktemp("cli_tally")
    blob = T.build_blob(T.every_type_entries())
    data = T.every_type_log()
    (d / "db.mxy").write_bytes(blob)
    (d / "in.log").write_bytes(data)
    want, n = T.oracle_counter(oracle, blob, data)
    assert len(want) > 22   # the default of 20 rows cuts
    return {"db": str(d / "db.mxy"), "log": str(d / "in.log"), "rows": T.ordered(want), "n": n}


def _run(args):
    return subprocess.run([str(CLI)] + args, capture_output=True, timeout=600)


def _rows(lines):
    recs = [json.loads(ln) for ln in lines]
    for ln, r in zip(lines, recs):
        assert list(r) == ["count", "item_type", "matched_text", "result"], ln   # sorted keys, nothing else
    return recs, [(r["matched_text"].encode(), r["item_type"], r["count"]) for r in recs]


def test_summary_prints_the_report_and_nothing_else(setup):
    for arg, limit in (("--tally=3", 3), ("--tally=0", 0), ("--tally", 20)):
        p = _run(["match", setup["db"], setup["log"], "--format", "summary", arg, "-s"])
        assert p.returncode == 0, p.stderr[-2000:]
        lines = p.stdout.decode().splitlines()
        want = setup["rows"][:limit] if limit else setup["rows"]
        assert len(lines) == len(want), arg
        _, got = _rows(lines)
        assert got == want, arg
        err = p.stderr.decode()
        assert "[INFO] Distinct matched values: %d" % len(setup["rows"]) in err and "[INFO] Total matches: %d" % setup["n"] in err.replace(",", "")


def test_json_prints_the_report_behind_the_matches_and_result_is_the_query(setup):
    plain = _run(["match", setup["db"], setup["log"], "--format", "json"])
    p = _run(["match", setup["db"], setup["log"], "--format", "json", "--tally"])
    assert plain.returncode == 0 and p.returncode == 0, p.stderr[-2000:]
    assert "Distinct matched values" not in p.stderr.decode()   # only with -s
    base = plain.stdout.decode().splitlines()
    lines = p.stdout.decode().splitlines()
    assert len(base) == setup["n"] and lines[:len(base)] == base   # the match records are what they were
    recs, got = _rows(lines[len(base):])
    assert got == setup["rows"][:20] and len(got) == 20
    for r in recs:
        q = _run(["query", setup["db"], r["matched_text"]])
        assert q.returncode == 0, r
        assert json.loads(q.stdout.decode()) == r["result"] and r["result"], r


def test_follow_with_tally_is_refused(setup):
    p = _run(["match", setup["db"], setup["log"], "--follow", "--tally"])
    assert p.returncode == 1 and p.stdout == b""
    assert "--tally is not supported with --follow" in p.stderr.decode()
    p = _run(["match", setup["db"], setup["log"], "--tally=x"])
    assert p.returncode == 2
