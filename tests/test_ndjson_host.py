"""CPU: the host NDJSON renderer (matchy_amd/csrc/ndjson_host.cpp) as a unit of its own, compiled with g++ under
-fsanitize=address,undefined into a stand-alone program (tests/cpp/test_ndjson_host.cpp) and compared with an assembly of the records
from json_escape, utf8_lossy_append, format_cidr(parse_ip()) and snprintf that never goes through render::record_emit. Every input
array and the batch text lie in heap blocks of exactly their length. No GPU."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "matchy_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ndjson_host") / "test_ndjson_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SAN, "-I", str(CSRC), str(ROOT / "tests" / "cpp" / "test_ndjson_host.cpp"),
                    str(CSRC / "ndjson_host.cpp"), str(CSRC / "data_codec.cpp"), "-o", str(exe), "-lpthread"], check=True)
    return exe


def run(driver, what, threads=None):
    env = dict(os.environ)
    env.pop("MATCHY_AMD_JSON_THREADS", None)
    if threads is not None:
        env["MATCHY_AMD_JSON_THREADS"] = str(threads)
    r = subprocess.run([str(driver), what], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "ndjson_host ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def test_the_unit_knows_neither_hip_nor_the_engine():
    for name in ("ndjson_host.h", "ndjson_host.cpp"):
        includes = set(re.findall(r'#include\s+"([^"]+)"', (CSRC / name).read_text()))
        assert includes <= {"../../include/matchy_amd.h", "ndjson_host.h", "render_core.h", "netaddr.h", "data_codec.h", "utf8_lossy.h"}, includes


def test_records_lines_segments_block_and_refusals(driver):
    """IPv4, IPv6 and compact records, an address that does not parse, pattern records with 0, 1, 3 and 4 ids and all, some and none of
    their offsets -1, a payload that does not decode, escapes in the matched text and ill-formed UTF-8 in the lines (the last one
    without a terminator), line bases, three sources of which one owns no record, every one of them from the batch and from the block
    of hit lines, and the single-record call on each record: 2 x (8 texts + 10 records)"""
    assert "cases=36" in run(driver, "cases")


def test_pieces_on_threads_give_the_bytes_of_one_thread(driver):
    """2 * 16384 + 1 records: two pieces under MATCHY_AMD_JSON_THREADS=4, one under =1; a payload first met by both pieces at once"""
    line = re.compile(r"big records=32769 bytes=(\d+) fnv=([0-9a-f]{16}) payload_555_calls=(\d+)")
    four, one = line.search(run(driver, "big", threads=4)), line.search(run(driver, "big", threads=1))
    assert four and one
    assert four.group(1, 2) == one.group(1, 2)
    assert (four.group(3), one.group(3)) == ("2", "1")
