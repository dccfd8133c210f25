"""CPU: the rules of the NDJSON renderer (matchy_amd/csrc/render_core.h) and the address formatters it shares with the host
(csrc/netaddr.h), compiled with g++ under -fsanitize=address,undefined as a stand-alone program (tests/cpp/test_render_core.cpp) and
compared with the host code the host renderer uses: utf8_lossy_append + json_escape, format_cidr(parse_ip()), snprintf. Every field
lies in a heap block of exactly its length and every output in a block of exactly the measured length. No GPU."""
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("render_core") / "test_render_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(CSRC), str(ROOT / "tests" / "cpp" / "test_render_core.cpp"),
                    str(CSRC / "data_codec.cpp"), "-o", str(exe)], check=True)
    return exe


def run(driver, what):
    r = subprocess.run([str(driver), what], capture_output=True, text=True)
    assert r.returncode == 0 and "render_core ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def test_escaping_whole_and_cut_at_every_position(driver):
    """every string of length <= 3 over the alphabet of edge bytes and every single byte, as matched_text and as input_line"""
    out = run(driver, "escape")
    assert int(re.search(r"escape strings=(\d+)", out).group(1)) == 21 + 21 ** 2 + 21 ** 3 + 256


def test_random_strings(driver):
    assert "random strings=10000" in run(driver, "random")


def test_a_byte_reads_three_back_and_three_ahead(driver):
    assert "window strings=2000" in run(driver, "window")


def test_addresses(driver):
    """IPv6 zero runs at every position and length, equal runs, a single zero group, ::, mapped, leading zeros, every prefix length;
    IPv4 at every prefix length; texts that do not parse"""
    out = run(driver, "ip")
    assert int(re.search(r"ip cases=(\d+)", out).group(1)) == 3 * 36 + 3 * 129 + 3 * 33 + 6


def test_decimal(driver):
    assert "decimal ok" in run(driver, "decimal")


def test_whole_records(driver):
    """IP and pattern records with every flag combination against a std::string assembly, at the exact capacity and below it"""
    assert "records=28" in run(driver, "records")
