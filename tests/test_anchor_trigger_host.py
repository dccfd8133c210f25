"""CPU: where k_anchor's front end needs the boundary plane and the long-token chain (matchy_amd/csrc/anchor_planes.h), compiled
with g++ and run over random blocks and the synthetic log shapes. No GPU."""
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

SHAPES = ("nginx", "ip-dense", "jsonl-app", "url-heavy", "hash-dense", "skewed-halves")   # all six; the last one with a period of 2000 lines
LINES = 40000


def test_boundary_plane_ipv4_plane_and_token_trigger(tmp_path):
    """boundary_plane() == classify_planes().B and lies inside the "neither digit nor '.'" plane for every byte value in every slot;
    the IPv4 anchor plane contains the one it replaced at every position (random bytes, random digits and dots) and lists not one
    anchor more on the first 40 000 lines of the six synthetic shapes; the token trigger is true in every
    block whose exact five-dword chain is nonzero and the exact chain equals a per-dword loop (a million random blocks at the densities
    0.3, 0.7 and 0.95, 100 000 more at 0.15, and the shapes); on the nginx shape the trigger fires in fewer than 25 % of the blocks (the exact
    chain is nonzero in 1.2 %, four dwords in a row stand in 44.9 %)."""
    from tools import synth
    exe = tmp_path / "test_anchor_trigger"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests/cpp/test_anchor_trigger.cpp"), "-o", str(exe)],
                   check=True)
    cfg = synth.config("c2")
    args = []
    for shape in SHAPES:
        f = tmp_path / (shape + ".log")
        f.write_bytes(synth.make_log(cfg, 0, LINES, shape, 2000 if shape == "skewed-halves" else 0))
        args.append(f"{shape}={f}")
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "anchor_trigger ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    for shape in SHAPES:
        m = re.search(rf"^{shape}: ipv4 anchors old (\d+) new (\d+); token trigger fires in (\d+) of (\d+) blocks", r.stdout, re.M)
        assert m, r.stdout[-4000:]
        old, new, fired, blocks = map(int, m.groups())
        assert new - old == 0, (shape, old, new)
        assert old > 0 or shape == "hash-dense", (shape, old)   # hash-dense holds no dotted text
        if shape == "nginx":
            assert fired * 100 < 25 * blocks, f"token trigger fires in {fired} of {blocks} nginx blocks = {100.0 * fired / blocks:.2f} %"
