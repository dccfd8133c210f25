"""What the UTF-16 front pass (csrc/utf16.hip) costs, and what `matchy match --encoding=utf-16le` buys over `iconv | matchy match`.

  pass   the UTF-16LE rendition of one batch of --mib MiB of nginx-style log (tools/synth, config c2: the BASELINE generator). Arms
         alternate repetition by repetition in one process: (A) the host-to-device copy of the UTF-16 batch from pinned memory, timed
         with events; (B) matchy_scanner_scan_utf16 of the batch resident in device memory, counters only; the three steps are timed by
         the library's own events (matchy_scanner_get_utf16_timing). Medians. The three steps together are expected to stay below the copy.
  cli    wall clock of whole processes on the same log as files, --format summary and --format json (stdout to /dev/null), arms
         alternating: (A) iconv -f UTF-16LE -t UTF-8 FILE | PARENT match DB -   — what a user does on the parent commit;
         (B) this tree: match DB FILE --encoding=utf-16le; (C) this tree and (D) the parent on the UTF-8 file without the flag: the
         default path did not move. --parent-cli: the parent commit's binary (this tree's when not given).

    python tools/utf16_timing.py [--parts pass,cli] [--reps R] [--mib N] [--parent-cli PATH] [--out FILE]"""
import argparse
import os
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


def make_inputs(mib):
    import numpy as np
    from tools import synth
    cfg = synth.config("c2")
    lines = mib * (1 << 20) // 190
    text = synth.make_log(cfg, 0, lines)
    u8 = np.frombuffer(text, dtype=np.uint8)
    assert int(u8.max()) < 0x80   # the generator writes ASCII: UTF-16LE is every byte followed by a zero
    u16 = np.zeros(2 * len(u8), dtype=np.uint8)
    u16[0::2] = u8
    return cfg, text, u16


def part_pass(reps, mib, out):
    import torch
    import matchy_amd as M
    from tools import synth
    cfg, text, u16 = make_inputs(mib)
    db = M.Database(synth.build_db(cfg))
    sc = M.Scanner(db)
    pinned = torch.empty(len(u16), dtype=torch.uint8).pin_memory()
    pinned.numpy()[:] = u16
    dev = torch.empty(len(u16) + 64, dtype=torch.uint8, device="cuda")
    dev[:len(u16)].copy_(pinned)
    torch.cuda.synchronize()
    want = sc.scan(text)
    want_hits, want_lines = want.n_hits, want.lines
    want.close()
    sc.scan_utf16(dev.data_ptr(), M.UTF16_LE, fetch_mode=0, nbytes=len(u16)).close()   # buffers grow here
    copies, steps, walls = [], [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev[:len(u16)].copy_(pinned, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        r = sc.scan_utf16(dev.data_ptr(), M.UTF16_LE, fetch_mode=0, nbytes=len(u16))
        walls.append((time.perf_counter() - t0) * 1e3)
        u = r.utf16()
        assert (u["text_len"], u["replaced"], r.n_hits, r.lines) == (len(text), 0, want_hits, want_lines)
        r.close()
        steps.append(sc.utf16_timing_ms())
    med = statistics.median
    count, prefix, write = (med(s[k] for s in steps) for k in range(3))
    copy = med(copies)
    out("pass: %d bytes of UTF-16LE -> %d bytes of UTF-8, %d hits; milliseconds, median of %d" % (len(u16), len(text), want_hits, reps))
    out("  host-to-device copy of the batch (pinned): %8.3f  (%.1f GB/s)" % (copy, len(u16) / copy / 1e6))
    out("  count  %8.3f  (%.0f GB/s of input)" % (count, len(u16) / count / 1e6))
    out("  prefix %8.3f" % prefix)
    out("  write  %8.3f  (%.0f GB/s of input + output)" % (write, (len(u16) + len(text)) / write / 1e6))
    out("  count + prefix + write %8.3f = %.2f of the copy" % (count + prefix + write, (count + prefix + write) / copy))
    out("  transcode + scan + fetch, wall clock of the call %8.3f" % med(walls))
    sc.close(); db.close()


def part_cli(reps, mib, parent_cli, out):
    from tools import synth
    cfg, text, u16 = make_inputs(mib)
    parent = str(parent_cli or CLI)
    d = Path(tempfile.mkdtemp(prefix="utf16_timing_"))
    try:
        (d / "db.mxy").write_bytes(synth.build_db(cfg))
        (d / "u8.log").write_bytes(text)
        (d / "u16.log").write_bytes(u16.tobytes())
        arms = {
            "A iconv | parent": "iconv -f UTF-16LE -t UTF-8 u16.log | %s match db.mxy - --format %%s" % parent,
            "B --encoding=utf-16le": "%s match db.mxy u16.log --encoding=utf-16le --format %%s" % CLI,
            "C UTF-8 file, this tree": "%s match db.mxy u8.log --format %%s" % CLI,
            "D UTF-8 file, parent": "%s match db.mxy u8.log --format %%s" % parent,
        }
        out("cli: %d bytes of UTF-8 / %d of UTF-16LE as files; wall clock seconds of the process, %d runs per arm, arms alternating" % (len(text), len(u16), reps))
        for fmt in ("summary", "json"):
            times = {k: [] for k in arms}
            for _ in range(reps):
                for k, cmd in arms.items():
                    t0 = time.perf_counter()
                    r = subprocess.run(["bash", "-o", "pipefail", "-c", cmd % fmt + " > /dev/null"], cwd=str(d), stderr=subprocess.PIPE)
                    times[k].append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr[-2000:]
            for k, v in times.items():
                out("  %-8s %-26s median %6.2f  min %6.2f  max %6.2f" % (fmt, k, statistics.median(v), min(v), max(v)))
            a, b = statistics.median(times["A iconv | parent"]), statistics.median(times["B --encoding=utf-16le"])
            c, dd = statistics.median(times["C UTF-8 file, this tree"]), statistics.median(times["D UTF-8 file, parent"])
            out("  %-8s B / A = %.2f   C / D = %.2f" % (fmt, b / a, c / dd))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pass,cli")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--parent-cli")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "utf16_timing.txt"))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("tools/utf16_timing.py --parts %s --reps %d --mib %d%s" % (a.parts, a.reps, a.mib, " --parent-cli (the parent commit's build)" if a.parent_cli else ""))
    if "pass" in a.parts:
        part_pass(a.reps, a.mib, out)
    if "cli" in a.parts:
        part_cli(max(3, a.reps // 2), a.mib, a.parent_cli, out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
