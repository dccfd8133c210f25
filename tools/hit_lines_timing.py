"""What the hit-lines pass (csrc/hit_lines.hip) costs and what `matchy match --gz-on-gpu --gather-lines` buys.

  pass   one batch of --lines nginx lines (tools/synth, config c2) resident in device memory, two databases: the headline's (c2: about
         one line in twenty hits) and "dense", a database of all 255 /8 networks under which every line hits — the worst case, text_len ~ len,
         standing in for the C5 batch (whose ten-million-entry database is not built here). Arms alternate repetition by repetition in
         one process: (A) the device-to-host copy of the WHOLE batch into pinned memory, timed with events — what a caller who renders
         records pays today; (B) the scan with hit lines, fetch mode 1, timed by matchy_scanner_get_hit_lines_timing: index steps (mark,
         rank, lengths, offsets), copy kernel, the block's device-to-host copy. Medians; the first scan of the scanner (whose block
         starts from an estimate and may regrow) is not among the repetitions.
  cli    the gz workload of tools/gz_inflate_timing.py: --files .gz files of 64 KiB of text, default JSON. Arm A: --parent-cli (the
         parent commit's binary; this tree's when not given) with --gz-on-gpu; arm B: this tree with --gz-on-gpu --gather-lines. Wall
         clock of the process, arms alternating; median, minimum, maximum.

    python tools/hit_lines_timing.py [--parts pass,cli] [--reps R] [--lines N] [--files N] [--parent-cli PATH] [--out FILE]"""
import argparse
import gzip
import json
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


def part_pass(reps, n_lines, out):
    import torch
    import matchy_amd as M
    from tools import synth
    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, n_lines)
    dense = M.DatabaseBuilder(build_epoch=1)
    for a in range(1, 256):
        dense.add_entry("%d.0.0.0/8" % a, {"k": "any"})
    blobs = (("headline", synth.build_db(cfg)), ("dense", dense.build()))
    dense.close()
    dlog = torch.empty(len(text) + 64, dtype=torch.uint8, device="cuda")
    dlog[:len(text)].copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    pinned = torch.empty(len(text), dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    out("pass: %d lines, %d bytes; device milliseconds, median of %d" % (n_lines, len(text), reps))
    out("%9s %10s %10s %11s %8s %8s %8s %8s %11s" % ("database", "hits", "hit lines", "block bytes", "index", "kernel", "d2h", "sum", "whole batch"))
    for name, blob in blobs:
        db = M.Database(blob)
        sc = M.Scanner(db, profile=True)
        sc.set_hit_lines(True)
        sc.scan_device(dlog.data_ptr(), len(text), stream=stream, fetch_mode=1).close()
        rows, whole = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pinned.copy_(dlog[:len(text)], non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            whole.append(e0.elapsed_time(e1))
            r = sc.scan_device(dlog.data_ptr(), len(text), stream=stream, fetch_mode=1)
            hl, t = r.hit_lines(), sc.hit_lines_timing_ms()
            rows.append((t["index"], t["copy_kernel"], t["d2h"]))
            hits, n, block = r.n_hits, hl["n_lines"], hl["text_len"]
            r.close()
        assert name != "dense" or n > n_lines // 2, "the dense database does not hit"
        index, kernel, d2h = (statistics.median(v) for v in zip(*rows))
        out("%9s %10d %10d %11d %8.3f %8.3f %8.3f %8.3f %11.3f" % (name, hits, n, block, index, kernel, d2h, index + kernel + d2h, statistics.median(whole)))
        sc.close(); db.close()


def part_cli(reps, n_files, parent_cli, out):
    from tools import synth
    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, 700)
    text = text[:text.rfind(b"\n", 0, 1 << 16) + 1]
    d = Path(tempfile.mkdtemp(prefix="hit_lines_timing_"))
    try:
        (d / "db.mxy").write_bytes(synth.build_db(cfg))
        data = gzip.compress(text, 6)
        paths = []
        for i in range(n_files):
            p = d / ("host%05d.log.gz" % i)
            p.write_bytes(data)
            paths.append(str(p))
        out("cli: %d .gz files of %d bytes of text each (%d compressed), default JSON, wall clock seconds of the process" % (n_files, len(text), len(data)))
        out("  arm A: %s --gz-on-gpu; arm B: this tree --gz-on-gpu --gather-lines" % ("the parent's binary" if parent_cli else "this tree (no parent binary given)"))
        arms = {"A": [], "B": []}
        sizes = {}
        for _ in range(reps):
            for arm, exe, flags in (("A", parent_cli or str(CLI), ["--gz-on-gpu"]), ("B", str(CLI), ["--gz-on-gpu", "--gather-lines"])):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "match", str(d / "db.mxy")] + paths + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
                arms[arm].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                sizes[arm] = (len(r.stdout), hash(r.stdout))
        assert sizes["A"] == sizes["B"], "the two arms print different records"
        for arm, v in arms.items():
            out("  %s median %.3f  min %.3f  max %.3f  (n = %d, %d bytes of NDJSON)" % (arm, statistics.median(v), min(v), max(v), len(v), sizes[arm][0]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pass,cli")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lines", type=int, default=2000000)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--parent-cli", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    if "pass" in a.parts:
        part_pass(a.reps, a.lines, out)
    if "cli" in a.parts:
        part_cli(a.reps, a.files, a.parent_cli, out)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
