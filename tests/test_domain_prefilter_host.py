"""CPU: the label-window rule of k_anchor's domain drain and the exact table of long-label prefixes behind it
(matchy_amd/csrc/domain_prefilter.h, hashes.h), compiled with g++ and run over the shipped public-suffix list, random and constructed
windows and the synthetic log shapes. No GPU."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = ("nginx", "url-heavy", "jsonl-app", "hash-dense", "ip-dense")
LINES = 40000
LONG_SURVIVORS_PERCENT = 3.5   # of a shape's long labels: the filter's rate (density 17.5 %, two probes: 3.1 %) plus margin


def test_label_window_rule_prefix_table_and_survivors(tmp_path):
    """Every last label of psl.bin is kept (every length, alignment and boundary byte); the exact table holds the 8-byte windows of the
    labels of 8 bytes or more and nothing else; the rule never keeps less than a byte-by-byte restatement of val_domain's first steps and
    agrees with it on dots and stop bytes (3.6 M windows); on the first 40 000 lines of five synthetic shapes the survivors with a short
    label are those of the rule it replaced, anchor by anchor, and the survivors with a long label are at most 3.5 % of the shape's long
    labels."""
    from tools import synth
    exe = tmp_path / "test_domain_prefilter"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests/cpp/test_domain_prefilter.cpp"), "-o", str(exe)],
                   check=True)
    cfg = synth.config("c2")
    args = [str(ROOT / "matchy_amd" / "data" / "psl.bin")]
    for shape in SHAPES:
        f = tmp_path / (shape + ".log")
        f.write_bytes(synth.make_log(cfg, 0, LINES, shape, 0))
        args.append(f"{shape}={f}")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "domain_prefilter ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    seen_long = 0
    for shape in SHAPES:
        m = re.search(rf"^{shape}: domain anchors (\d+); short labels (\d+) survivors old (\d+) new (\d+) differing (\d+); "
                      r"long labels (\d+) survivors old (\d+) new (\d+) listed (\d+)", r.stdout, re.M)
        assert m, r.stdout[-4000:]
        anchors, short_n, short_old, short_new, short_diff, long_n, long_old, long_new, long_listed = map(int, m.groups())
        assert short_diff == 0 and short_old == short_new, (shape, short_old, short_new, short_diff)
        assert long_new * 100 <= LONG_SURVIVORS_PERCENT * long_n, f"{shape}: {long_new} of {long_n} long labels survive = {100.0 * long_new / max(1, long_n):.2f} %"
        assert anchors > 0 or shape == "ip-dense", shape   # addresses only
        seen_long += long_n
    assert seen_long > 100000   # url-heavy alone has more
