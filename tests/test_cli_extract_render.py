"""GPU: `matchy extract --render-on-gpu` prints byte for byte what the command prints without the flag — the items of a batch are put
into line order and written as json / csv / text on the GPU (csrc/extract_render.hip) in place of the per-item work of extract_batch —
and reports the same figures with --stats."""
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import distinct_cases as D   # noqa: E402

pytestmark = pytest.mark.gpu

OPTIONS = {"plain": [], "unique": ["--unique"], "types": ["--types", "ip,domain"], "min_labels": ["--min-labels", "3"]}


@pytest.fixture(scope="module")
def cli():
    import matchy_amd.build as B
    B.build()
    assert B.CLI.exists()
    return str(B.CLI)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Two files and a third input for stdin, each many 4 KiB batches long, with overlapping values; CRLF lines, empty and blank lines, form
    feeds in the margins and inside lines, a value with a quote and a backslash next to it, and a last line without a newline."""
    import random
    rng = random.Random(78)
    texts = D.basic_texts(rng)
    odd = (b'q "quoted.example.com" \\back.example.org\\ "\\10.20.30.40\\"\r\n'
           b"\r\n\n   \t \n"
           b"\x0c\x0c margin.example.net 10.1.1.1 \x0c\n"
           b"inside 10.2.2.2\x0cform.example.net\x0c172.16.0.9 feed\r\n"
           b" \x0c\r\n")
    d = tmp_path_factory.mktemp("xrender")
    a, b = d / "a.log", d / "b.log"
    log_a = D.make_log(rng, texts[:200], 500, heavy="10.0.0.1", heavy_share=0.3).replace(b" ok\n", b" ok\r\n")
    a.write_bytes(log_a[:len(log_a) // 2] + odd + log_a[len(log_a) // 2:])
    b.write_bytes(D.make_log(rng, texts[100:], 500, heavy="10.0.0.1", heavy_share=0.3) + b"tail.example.com 192.0.2.77 without a newline")
    piped = odd + D.make_log(rng, texts[50:250], 300) + b"\n\n"
    return [str(a), "-", str(b)], piped


def _run(args, piped, status=0):
    r = subprocess.run(args, input=piped, capture_output=True, timeout=300)
    assert r.returncode == status, r.stderr[-2000:]
    return r.stdout, r.stderr.decode()


def _info(err):
    return [l for l in err.splitlines() if not l.startswith(("[INFO] Throughput:", "[INFO] Total time:"))]


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("batch", ["4096", "default"])
@pytest.mark.parametrize("fmt", ["json", "csv", "text"])
def test_same_output_as_the_host_path(cli, inputs, fmt, batch, option):
    files, piped = inputs
    base = [cli, "extract", *files, "--format", fmt, "--stats", *OPTIONS[option]] + (["--batch-bytes", batch] if batch != "default" else [])
    want, want_err = _run(base, piped)
    got, got_err = _run(base + ["--render-on-gpu"], piped)
    assert len(want.splitlines()) > (100 if option != "plain" else 1000)
    assert got == want
    info = _info(want_err)
    assert _info(got_err) == info
    assert any(l.startswith("[INFO] Patterns found:") for l in info) and any(l.startswith("[INFO] Lines processed:") for l in info)


def test_show_candidates_is_refused(cli, inputs):
    files, piped = inputs
    out, err = _run([cli, "extract", *files, "--render-on-gpu", "--show-candidates"], piped, status=1)
    assert out == b"" and len(err.splitlines()) == 1 and "--show-candidates" in err


def test_flag_order_and_equals_forms(cli, inputs):
    files, piped = inputs
    want, _ = _run([cli, "extract", "--format=csv", *files], piped)
    got, _ = _run([cli, "extract", "--render-on-gpu", "--format=csv", *files], piped)
    assert got == want and got.startswith(b"type,value\n")
