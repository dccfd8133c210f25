"""What pieces of one stream (csrc/inflate_pieces.hip, `matchy match --gz-on-gpu --gz-pieces`) cost and buy, on the headline log shape
(tools/synth: config c2, nginx lines), one GPU, medians of --reps.

  one    (a) one member of 1, 16 and 64 MiB of text at gzip level 6: device milliseconds of the inflate stage with pieces off and with
         piece_bytes of 4, 8, 16, 32 and 64 KiB, and the per-kernel times of matchy_scanner_get_gz_pieces_timing.
         (b) the same files through zlib on one core in the same run (what gzread costs: the host path the flag replaces).
  pack   (c) 64 files of 16 MiB of text in one pack, pieces off and on.
  cli    (d) the command line on one .gz of 64 MiB of text in the page cache, without flags (arm A: gzread) and with --gz-on-gpu
         --gz-pieces (arm B); wall clock of the process, the arms alternate repetition by repetition.
  (e), the default path, is bench.py on this tree and on the parent commit's tree, run side by side by the caller.

    python tools/gz_pieces_timing.py [--parts one,pack,cli] [--reps R] [--out FILE]"""
import argparse
import gzip
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
PIECES = (4096, 8192, 16384, 32768, 65536)
KERNELS = ("find", "count", "chain", "symbols", "resolve", "handover")


def headline(nbytes):
    """(database blob, about nbytes of the headline log, cut at a line end)"""
    from tools import synth
    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, max(100, nbytes // 100))
    assert len(text) >= nbytes, "raise the line estimate"
    return synth.build_db(cfg), text[:text.rfind(b"\n", 0, nbytes) + 1]


def timed_scan(sc, blobs, piece_bytes, reps):
    """medians: (inflate stage ms, {kernel: ms}), and the live / all pieces and the members handed over of the last repetition"""
    sc.set_gz_pieces(piece_bytes)
    stage, parts, census = [], [], (0, 0, 0)
    for _ in range(reps):
        r = sc.scan_gz(blobs, fetch_mode=0)
        assert all(s == 0 for s in r.gz_status()), "a member failed"
        stage.append(sc.gz_timing_ms()["inflate"])
        parts.append(sc.gz_pieces_timing_ms())
        pieces, first = r.gz_pieces()
        if pieces:
            handed = sum(1 for i in range(len(blobs)) if first[i + 1] > first[i] and pieces[first[i]][5] & 4)
            census = (sum(1 for p in pieces if p[5] & 2), len(pieces), handed)
        r.close()
    return statistics.median(stage), {k: statistics.median(p[k] for p in parts) for k in KERNELS}, census


def part_one(reps, out):
    import matchy_amd as M
    blob, _ = headline(1 << 16)
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    out("one member, level 6: device milliseconds of the inflate stage, median of %d; zlib = one core, same run" % reps)
    out("%9s %9s %7s %9s %8s | %8s %8s %8s %8s %8s %8s | %11s" % ("text", "packed", "pieces", "inflate", "GB/s", *KERNELS, "live/all/ho"))
    for size in (1 << 20, 1 << 24, 1 << 26):
        _, text = headline(size)
        gz = gzip.compress(text, 6)
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = zlib.decompress(gz, 31)
            host.append((time.perf_counter() - t0) * 1e3)
        assert got == text
        out("%9d %9d %7s %9.3f %8.3f" % (len(text), len(gz), "zlib", statistics.median(host), len(text) / statistics.median(host) / 1e6))
        for pb in (0,) + PIECES:
            ms, parts, census = timed_scan(sc, [gz], pb, reps)
            out("%9d %9d %7d %9.3f %8.3f | %s | %d/%d/%d" % (len(text), len(gz), pb, ms, len(text) / ms / 1e6, " ".join("%8.3f" % parts[k] for k in KERNELS), *census))
    sc.close(); db.close()


def part_pack(reps, out):
    import matchy_amd as M
    blob, text = headline(1 << 24)
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    gz = gzip.compress(text, 6)
    out("pack of 64 files of %d bytes of text (%d compressed): inflate stage ms, median of %d" % (len(text), len(gz), reps))
    for pb in (0, 8192, 65536):
        ms, parts, census = timed_scan(sc, [gz] * 64, pb, reps)
        out("%7d %9.3f ms %8.3f GB/s | %s | %d/%d/%d" % (pb, ms, 64 * len(text) / ms / 1e6, " ".join("%8.3f" % parts[k] for k in KERNELS), *census))
    sc.close(); db.close()


def part_cli(reps, piece_bytes, out):
    blob, text = headline(1 << 26)
    d = Path(tempfile.mkdtemp(prefix="gz_pieces_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        (d / "access.log.gz").write_bytes(gzip.compress(text, 6))
        out("cli: one .gz of %d bytes of text (%d compressed), --format summary, wall clock seconds of the process" % (len(text), (d / "access.log.gz").stat().st_size))
        arms = {"gzread": [], "gz-pieces": []}
        outs = {}
        for _ in range(reps):
            for arm, flags in (("gzread", []), ("gz-pieces", ["--gz-on-gpu", "--gz-pieces=%d" % piece_bytes])):
                t0 = time.perf_counter()
                r = subprocess.run([str(CLI), "match", str(d / "db.mxy"), str(d / "access.log.gz"), "--format", "summary"] + flags, capture_output=True, timeout=600)
                arms[arm].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                outs[arm] = r.stdout
        assert outs["gzread"] == outs["gz-pieces"]
        for arm, v in arms.items():
            out("  %-10s median %.3f  min %.3f  max %.3f  (n = %d)" % (arm, statistics.median(v), min(v), max(v), len(v)))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="one,pack,cli")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cli-piece-bytes", type=int, default=8192)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            Path(a.out).write_text("\n".join(lines) + "\n")
    if "one" in a.parts:
        part_one(a.reps, out)
    if "pack" in a.parts:
        part_pack(a.reps, out)
    if "cli" in a.parts:
        part_cli(a.reps, a.cli_piece_bytes, out)
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
