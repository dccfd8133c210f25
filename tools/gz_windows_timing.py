"""What `matchy match --gz-on-gpu --gz-members --gz-windows` buys on ONE multi-member .gz file that is larger than a batch, on the headline
log shape (tools/synth: config c2, nginx lines), and what the window's own kernel costs.

  tail   k_gz_window_tail alone (matchy_scanner_get_gz_window_timing, HIP events) through matchy_scanner_scan_gz_window, counts only:
         (typical) a window of 4 096 BGZF-style members of 64 KiB of text that ends in the middle of a log line, carry_cap 1 MiB — beside
                   it inflate (CRC included) and verdict + seal + tail of the same window, and GB/s of inflated text;
         (worst)   a small window whose last line has exactly carry_cap = 1 MiB bytes and no newline: the walk goes back through all of
                   it, and all of it is copied out and blanked.
  cli    `--format summary` wall clock of the process, page cache warm, default --batch-bytes, one BGZF-style file of --gib GiB of text:
         arm A = this tree WITHOUT gz flags (the gzread path of read_input), arm B = the three flags. The arms alternate repetition by
         repetition; median, minimum, maximum.

The text is 16 MiB of the log repeated, so that every distinct member is compressed once (level 6).
NOT measured here: a cold page cache, more than one GPU, JSON output.

    python tools/gz_windows_timing.py [--parts tail,cli] [--reps R] [--gib N] [--out FILE]"""
import argparse
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
sys.path.insert(0, str(ROOT / "tools"))
from gz_members_timing import CLI, headline, member   # noqa: E402

CARRY_CAP = 1 << 20
FLAGS = ["--gz-on-gpu", "--gz-members", "--gz-windows"]


def bgzf_members(text, block=1 << 16):
    return b"".join(member(text[i:i + block], True) for i in range(0, len(text), block))


def part_tail(blob, unit, reps, out):
    import matchy_amd as M
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    out("tail: device milliseconds, median of %d (inflate includes the CRC; verdict+seal+tail = k_gz_file_verdict + k_gz_seal_files + k_gz_window_tail; tail = k_gz_window_tail alone)" % reps)
    out("%8s %8s %11s %9s %10s %18s %9s %9s" % ("window", "members", "text", "tail len", "inflate", "verdict+seal+tail", "tail", "GB/s"))
    cut = unit.rfind(b"\n") - 40                                   # the window ends 40 bytes in front of a line end: inside a log line
    typical = bgzf_members(unit[:cut]) * 15 + bgzf_members(unit[:cut])   # 16 x 16 MiB: about 4 096 members, ends mid-line
    head = unit[:unit.find(b"\n", 1 << 16) + 1]
    worst = bgzf_members(head + b"x" * CARRY_CAP)
    for name, data in (("typical", typical), ("worst", worst)):
        ms, tail_len, n = [], 0, 0
        for _ in range(reps):
            r = sc.scan_gz_window(data, carry_cap=CARRY_CAP, fetch_mode=0)
            status, carry = r.gz_window()
            assert r.gz_file_status() == [0] and status == 0, "the window failed"
            tail_len, n, text_len = len(carry), len(r.gz_status()), r.gz_text_len()
            t = sc.gz_window_timing_ms()
            ms.append((t["inflate"], t["seal"], t["tail"]))
            r.close()
        inflate, seal, tail = (statistics.median(v) for v in zip(*ms))
        out("%8s %8d %11d %9d %10.3f %18.3f %9.3f %9.3f" % (name, n, text_len, tail_len, inflate, seal, tail, text_len / (inflate + seal) / 1e6))
    sc.close(); db.close()


def part_cli(blob, unit, gib, reps, out):
    d = Path(tempfile.mkdtemp(prefix="gz_windows_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        one = bgzf_members(unit)
        repeats = gib * 64
        p = d / "big.log.gz"
        with open(p, "wb") as f:
            for _ in range(repeats):
                f.write(one)
            f.write(member(b"", True))
        text_len = len(unit) * repeats
        out("cli: one BGZF-style .gz file of %d bytes of text (%d compressed), --format summary, default --batch-bytes, wall clock seconds of the process" % (text_len, p.stat().st_size))
        out("     arm A = this tree without gz flags (gzread on the reader thread), arm B = --gz-on-gpu --gz-members --gz-windows")
        arms = {"A gzread": [], "B gz-windows": []}
        where, counts = "", {}
        for _ in range(reps):
            for arm, flags in (("A gzread", []), ("B gz-windows", FLAGS)):
                t0 = time.perf_counter()
                r = subprocess.run([str(CLI), "match", str(d / "db.mxy"), str(p), "--format", "summary", "-s"] + flags, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
                arms[arm].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr[-2000:]
                counts[arm] = re.findall(rb"\[INFO\] (Lines processed|Total matches): ([\d,]+)", r.stderr)
                if flags:
                    m = re.search(rb"gz windows on the GPU: (\d+) windows of (\d+) files, (\d+) finished on the host", r.stderr)
                    where = "%s windows of %s file(s), %s finished on the host" % tuple(x.decode() for x in m.groups()) if m else "?"
        assert counts["A gzread"] == counts["B gz-windows"], counts
        for arm, v in arms.items():
            out("  %-13s median %.3f  min %.3f  max %.3f  (n = %d)  %.2f GB/s of text" % (arm, statistics.median(v), min(v), max(v), len(v), text_len / statistics.median(v) / 1e9))
        out("  arm B: %s; both arms count %s" % (where, ", ".join("%s %s" % (k.decode(), v.decode()) for k, v in counts["A gzread"])))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="tail,cli")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gib", type=int, default=2, help="GiB of text of the command-line file")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    blob, unit = headline(16 << 20)
    if "tail" in a.parts:
        part_tail(blob, unit, a.reps, out)
    if "cli" in a.parts:
        part_cli(blob, unit, a.gib, a.reps, out)
    out("not measured: a cold page cache, more than one GPU, JSON output")
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
