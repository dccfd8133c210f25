"""CPU: the packing decisions of `matchy match --gz-on-gpu` (matchy_amd/csrc/gz_packer.h: the bounds, the eligibility of one input, the
pack in hand), compiled with g++ under -fsanitize=address,undefined as a stand-alone program and held, line for line, against the
Python model of tests/gz_packer_cases.py. No GPU."""
import subprocess
from pathlib import Path

import pytest

import gz_packer_cases as P

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SCENARIOS = dict(P.scenarios())
BB, MM = P.BATCH, P.MAX_MEMBER


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gz_packer") / "test_gz_packer"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(ROOT / "matchy_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "test_gz_packer.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def drive(driver, batch_bytes, members, args, max_member=None, max_carry=None):
    """(the four bounds, the lines behind them)"""
    opt = ["-" if v is None else str(v) for v in (max_member, max_carry)]
    r = subprocess.run([str(driver), str(batch_bytes), str(int(members)), *opt, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("bounds ")
    return tuple(map(int, lines[0].split()[1:])), lines[1:]


def lay_out(tmp_path, inputs):
    args = []
    for i, inp in enumerate(inputs):
        path = tmp_path / ("%02d_%s" % (i, inp.name))
        if inp.kind == "dir":
            path.mkdir()
        elif inp.kind == "file":
            path.write_bytes(inp.data)
        args.append(("!" if inp.shrinks else "") + str(path))
    return args


@pytest.mark.parametrize("members", [False, True])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_the_packer_agrees_with_its_model(driver, tmp_path, name, members):
    inputs = SCENARIOS[name]
    got_bounds, got = drive(driver, BB, members, lay_out(tmp_path, inputs))
    assert got_bounds == P.bounds(BB) == (BB, MM, MM, BB - MM)
    assert got == P.run(inputs, BB, members)
    seen = sorted(int(w.split(":")[0]) for ln in got for w in ln.split()[1:])
    assert seen == list(range(len(inputs)))                   # every input exactly once, and in input order
    assert [int(w.split(":")[0]) for ln in got for w in ln.split()[1:]] == seen


def packs(lines):
    return [[tuple(map(int, w.split(":"))) for w in ln.split()[1:]] for ln in lines if ln.startswith("pack ")]


def singles(lines):
    return [int(ln.split()[1]) for ln in lines if ln.startswith("single ")]


def test_the_scenarios_reach_the_edges_they_are_named_for():
    """on the model, which the driver is held to above: the figures a reader can check by hand"""
    for members in (False, True):
        lines = P.run(SCENARIOS["length_and_header"], BB, members)
        assert singles(lines) == [1, 3, 4, 6]                 # 17 bytes, two headers that do not parse, 7 bytes for the trailer
        assert any(f[0] == 2 and f[2:] == (18, 5, 1) for p in packs(lines) for f in p) and any(f[0] == 7 and f[2] == 25 for p in packs(lines) for f in p)
        assert singles(P.run(SCENARIOS["name_and_type"], BB, members)) == [3, 5, 7, 8]
        lines = P.run(SCENARIOS["member_bounds"], BB, members)
        assert singles(lines) == [1, 3]
        flat = [f for p in packs(lines) for f in p]
        assert flat[0][2] == MM and flat[1][3] == MM          # compressed size and ISIZE exactly at the bound stay
        (one, other) = packs(P.run(SCENARIOS["text_exactly_batch_bytes"], BB, members))
        assert [f[0] for f in one] == [0, 1, 2, 3] and sum(f[3] + 1 for f in one) == BB and [f[0] for f in other] == [4]
        (one, other) = packs(P.run(SCENARIOS["text_one_byte_more"], BB, members))
        assert [f[0] for f in one] == [0, 1, 2] and [f[0] for f in other] == [3, 4] and sum(f[3] + 1 for f in one) + other[0][3] + 1 == BB + 1
        lines = P.run(SCENARIOS["shrinks"], BB, members)
        assert singles(lines) == [2, 4] and [[f[0] for f in p] for p in packs(lines)] == [[0, 1], [3], [5]]
    lines = P.run(SCENARIOS["members"], BB, True)
    assert singles(lines) == [3, 4, 5, 8, 9, 10]
    got = packs(lines)
    assert [[f[0] for f in p] for p in got] == [[0, 1], [2], [6], [7], [11, 12, 13]]
    assert got[0][0][4] == 2 and got[0][1][2:] == (3000, 0, 150)       # 3000 + 2000 compressed bytes do not share a pack, whatever their text
    assert got[1][0][2:] == (2000, 0, 100)
    assert got[2][0][3:] == (BB - 1, 4)                               # sum + 1 == batch_bytes fits, and fills the pack
    assert got[4][0][4] > 5 and got[4][1][4] == 1
    lines = P.run(SCENARIOS["members"], BB, False)
    # without members mode a file is judged as one member, by its whole size and its last trailer: only what is above max_member leaves
    assert len(SCENARIOS["members"][11].data) > MM            # the BGZF file: ten blocks and their 26 bytes of container each
    assert singles(lines) == [1, 2, 3, 5, 9, 10, 11] and all(f[4] == 1 for p in packs(lines) for f in p)


def test_bounds(driver):
    cases = [(BB, None, None), (1 << 28, None, None), (1 << 28, 1000, None), (1 << 28, None, 77), (1 << 28, 5000, 100), (1 << 28, 1 << 40, 1 << 40),
             (1 << 28, 1 << 27, 1 << 21), (BB, 100, 200), (BB, 0, None), (1 << 31, None, None), ((1 << 31) + 12345, None, None), (1 << 40, 1 << 20, None)]
    for bb, mm, cc in cases:
        got, rest = drive(driver, bb, False, [], mm, cc)
        assert got == P.bounds(bb, mm, cc) and rest == [], (bb, mm, cc)
    assert P.bounds(1 << 28) == (1 << 28, 1 << 26, 1 << 20, (1 << 28) - (1 << 20))
    assert P.bounds(1 << 28, 1000, None) == (1 << 28, 1000, 1000, (1 << 28) - 1000)          # a lower max_member lowers the carry with it
    assert P.bounds(1 << 28, 1 << 40, 1 << 40) == P.bounds(1 << 28)                           # higher overrides are ignored
    assert P.bounds(1 << 40)[0] == P.bounds((1 << 31) + 12345)[0] == (1 << 31) - (1 << 20)    # a batch stays below 2^31


def test_the_header_is_host_only():
    src = (ROOT / "matchy_amd" / "csrc" / "gz_packer.h").read_text()
    assert "hip/" not in src and "matchy_amd.h" not in src
