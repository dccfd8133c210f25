"""What windows of one stream (csrc/inflate_pieces.hip "stream windows", `matchy match --gz-on-gpu --gz-pieces --gz-stream-windows`) cost
and buy: ONE single-stream .gz of the headline log shape (tools/synth: config c2, nginx lines; 32 MiB generated, laid end to end to
--text-mib), gzip level 6, several times --batch-mib, page cache warm, one GPU.

  cli     wall clock of the process without gz flags (arm A: gzread on one core, the path the flag replaces) and with the three flags
          (arm B), for --format summary, NDJSON, --render-on-gpu and --gather-lines; the arms alternate repetition by repetition;
          median, min and max of --reps. stdout of the two arms is compared.
  passes  the chain through Scanner.scan_gz_stream with profiling on, windows as csrc/gz_stream.h walks them at the command line's
          sizes: per-pass device milliseconds (matchy_scanner_get_gz_stream_timing) summed over the windows, median of --reps chains.
  The default path is bench.py on this tree and on the parent commit's tree, run side by side by the caller.

    python tools/gz_stream_timing.py [--parts cli,passes] [--reps R] [--text-mib N] [--batch-mib N] [--out FILE]"""
import argparse
import gzip
import json
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
FLAGS = ["--gz-on-gpu", "--gz-pieces", "--gz-stream-windows"]
PIECE_BYTES = 8192          # the default of --gz-pieces
CARRY_CAP = 1 << 20         # gz_packer.h gz_bounds
MODES = (("summary", ["--format", "summary"]), ("ndjson", []), ("render-on-gpu", ["--render-on-gpu"]), ("gather-lines", ["--gather-lines"]))


def headline(nbytes):
    """(database blob, nbytes of the headline log, cut at a line end): 32 MiB generated, repeated"""
    from tools import synth
    cfg = synth.config("c2")
    unit = min(nbytes, 32 << 20)
    text = synth.make_log(cfg, 0, max(100, unit // 100))
    assert len(text) >= unit, "raise the line estimate"
    text = text[:text.rfind(b"\n", 0, unit) + 1]
    return synth.build_db(cfg), text * max(1, nbytes // len(text))


def part_cli(d, batch, reps, out):
    base = [str(CLI), "match", str(d / "db.mxy"), str(d / "access.log.gz"), "--batch-bytes", str(batch), "-s"]
    for mode, mflags in MODES:
        arms, outs, stat = {"no flags": [], "stream windows": []}, {}, b""
        for _ in range(reps):
            for arm, flags in (("no flags", []), ("stream windows", FLAGS)):
                t0 = time.perf_counter()
                r = subprocess.run(base + mflags + flags, capture_output=True, timeout=900)
                arms[arm].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                outs[arm] = r.stdout
                if flags:
                    stat = re.search(rb"gz stream windows on the GPU: [^\n]*", r.stderr).group(0)
        assert outs["no flags"] == outs["stream windows"], mode
        out("cli %s (%d bytes of stdout; %s)" % (mode, len(outs["no flags"]), stat.decode()))
        for arm, v in arms.items():
            out("  %-15s median %.3f  min %.3f  max %.3f  (n = %d)" % (arm, statistics.median(v), min(v), max(v), len(v)))


def part_passes(blob, gz, text_len, batch, reps, out):
    import matchy_amd as M
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    sc.set_gz_pieces(PIECE_BYTES)
    text_cap = batch - CARRY_CAP - 1
    window_bytes = min(batch, text_cap)
    chains, walls, n_windows = [], [], 0
    for _ in range(reps):
        walk = M.GzStreamWalker(len(gz), window_bytes, PIECE_BYTES, text_cap, window_bytes // 4)
        state, carry, total, done = None, b"", dict.fromkeys(M.GZ_STREAM_PASSES, 0.0), 0
        t0 = time.perf_counter()
        while not walk.over:
            w = walk.next()
            r = sc.scan_gz_stream(gz[w[0]:w[0] + w[1]], state=state, carry=carry, carry_cap=CARRY_CAP, text_cap=text_cap, first=bool(w[3] & 1), file_end=bool(w[3] & 2),
                                  fetch_mode=0)
            v = r.gz_stream()
            done += r.bytes
            r.close()
            assert v["status"] == 0, v
            for k, ms in sc.gz_stream_timing_ms().items():
                total[k] += ms
            walk.accept(w, v["consumed_bits"], v["text_len"], v["ended"])
            state, carry = v["state"], v["carry"]
        walls.append(time.perf_counter() - t0)
        assert walk.ended and done == text_len
        chains.append(total)
        n_windows = walk.windows
    med = {k: statistics.median(c[k] for c in chains) for k in M.GZ_STREAM_PASSES}
    out("passes: %d windows, text_cap %d, pieces of %d; device ms summed over the windows, median of %d chains (counts only, profiling on)" % (n_windows, text_cap, PIECE_BYTES, reps))
    out("  " + "  ".join("%s %.1f" % kv for kv in med.items()))
    out("  all passes %.1f ms = %.2f GB/s of text; wall clock of the chain %.3f s (min %.3f, max %.3f), inflate, scan and round trips" %
        (sum(med.values()), text_len / sum(med.values()) / 1e6, statistics.median(walls), min(walls), max(walls)))
    sc.close(); db.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="cli,passes")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--text-mib", type=int, default=128)
    ap.add_argument("--batch-mib", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            Path(a.out).write_text("\n".join(lines) + "\n")
    blob, text = headline(a.text_mib << 20)
    gz = gzip.compress(text, 6)
    batch = a.batch_mib << 20
    out("one single-stream .gz: %d bytes of text, %d compressed (level 6, %.1f : 1), --batch-bytes %d" % (len(text), len(gz), len(text) / len(gz), batch))
    d = Path(tempfile.mkdtemp(prefix="gz_stream_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        (d / "access.log.gz").write_bytes(gz)
        if "cli" in a.parts:
            part_cli(d, batch, a.reps, out)
        if "passes" in a.parts:
            part_passes(blob, gz, len(text), batch, a.reps, out)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
