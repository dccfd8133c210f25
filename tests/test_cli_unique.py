"""GPU: `matchy extract --unique` prints the first occurrence of every value, across batches and input files — the handle's device set
(csrc/distinct.hip) replaced the host-side lookups of the command line."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distinct_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert B.CLI.exists()
    return str(B.CLI)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Two files with overlapping values, each many 4 KiB batches long; a value with a quote and a backslash next to it for the escapes."""
    import random
    rng = random.Random(77)
    texts = D.basic_texts(rng)
    d = tmp_path_factory.mktemp("uniq")
    a, b = d / "a.log", d / "b.log"
    a.write_bytes(D.make_log(rng, texts[:200], 700, heavy="10.0.0.1", heavy_share=0.3) + b'q "quoted.example.com" \\back.example.org\n')
    b.write_bytes(D.make_log(rng, texts[100:], 700, heavy="10.0.0.1", heavy_share=0.3))
    return [str(a), str(b)]


def _run(args):
    r = subprocess.run(args, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.decode().splitlines(), r.stderr.decode()


@pytest.mark.parametrize("fmt", ["json", "csv", "text"])
def test_unique_output_is_the_plain_output_filtered_by_first_occurrence(cli, inputs, fmt):
    base = [cli, "extract", *inputs, "--format", fmt, "--batch-bytes", "4096"]
    plain, _ = _run(base)
    got, err = _run(base + ["--unique", "--stats"])
    head = plain[:1] if fmt == "csv" else []
    body = plain[len(head):]
    # the printed value is the candidate's text: the whole line for text, behind the type for json / csv
    value = {"text": lambda l: l, "json": lambda l: l.split('"value":', 1)[1], "csv": lambda l: l.split(",", 1)[1]}[fmt]
    seen, want = set(), []
    for line in body:
        v = value(line)
        if v not in seen:
            seen.add(v)
            want.append(line)
    assert len(body) > 1200 and len(want) < len(body) // 3
    assert got == head + want
    m = re.search(r"\[INFO\] Patterns found: ([\d,]+)", err)
    assert m and int(m.group(1).replace(",", "")) == len(want)
    assert "[INFO] Unique mode: true" in err
