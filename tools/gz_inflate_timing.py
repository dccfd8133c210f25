"""What the gz pass (csrc/inflate.hip) costs and what `matchy match --gz-on-gpu` buys, on the headline log shape (tools/synth: config c2,
nginx lines).

  pass   packs of 1, 64, 1 024 and 16 384 copies of one gzip file of 64 KiB, 1 MiB and 16 MiB of text at gzip levels 1, 6 and 9 (packs whose
         text would reach 2^31 bytes are skipped): device time of inflate (+ CRC, fused) and seal from matchy_scanner_get_gz_timing, GB/s of
         inflated text per pack, the rate of ONE wave (the one-member pack), and the scan's own device time beside them.
  cli    a directory of --files .gz files of 64 KiB of text in the page cache: `--format summary` and the default JSON, without the flag
         (arm A: the gzread path of read_input, which this change does not touch) and with --gz-on-gpu (arm B). Wall clock of the
         process; the arms alternate repetition by repetition; median, minimum and maximum.

    python tools/gz_inflate_timing.py [--parts pass,cli] [--reps R] [--files N] [--out FILE]"""
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


def headline(nbytes):
    """(database blob, about nbytes of the headline log, cut at a line end)"""
    from tools import synth
    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, max(100, nbytes // 100))
    assert len(text) >= nbytes, "raise the line estimate"
    return synth.build_db(cfg), text[:text.rfind(b"\n", 0, nbytes) + 1]


def part_pass(reps, out):
    import matchy_amd as M
    blob, _ = headline(1 << 16)
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    out("pass: device milliseconds, median of %d (inflate includes the CRC; scan = the scan's own total)" % reps)
    out("%9s %5s %7s %9s %9s %9s %9s %9s %9s" % ("text", "level", "members", "ratio", "inflate", "seal", "scan", "GB/s", "hits"))
    for size in (1 << 16, 1 << 20, 1 << 24):
        _, text = headline(size)
        for level in (1, 6, 9):
            gz = gzip.compress(text, level)
            for n in (1, 64, 1024, 16384):
                if n * (len(text) + 1) >= (1 << 31):
                    continue
                ms = []
                for _ in range(reps):
                    r = sc.scan_gz([gz] * n, fetch_mode=0)
                    assert all(s == 0 for s in r.gz_status()), "a member failed"
                    t, hits = sc.gz_timing_ms(), r.n_hits
                    ms.append((t["inflate"], t["seal"], sc.timing_ms()["total"]))
                    r.close()
                inflate, seal, scan = (statistics.median(v) for v in zip(*ms))
                out("%9d %5d %7d %9.2f %9.3f %9.3f %9.3f %9.3f %9d" % (len(text), level, n, len(text) / len(gz), inflate, seal, scan,
                                                                  n * len(text) / inflate / 1e6 if inflate else 0.0, hits))
    sc.close(); db.close()


def part_cli(reps, n_files, out):
    blob, text = headline(1 << 16)
    d = Path(tempfile.mkdtemp(prefix="gz_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        data = gzip.compress(text, 6)
        paths = []
        for i in range(n_files):
            p = d / ("host%05d.log.gz" % i)
            p.write_bytes(data)
            paths.append(str(p))
        out("cli: %d .gz files of %d bytes of text each (%d compressed), wall clock seconds of the process" % (n_files, len(text), len(data)))
        for fmt in ("summary", "json"):
            arms = {"gzread": [], "gz-on-gpu": []}
            for _ in range(reps):
                for arm, flags in (("gzread", []), ("gz-on-gpu", ["--gz-on-gpu"])):
                    t0 = time.perf_counter()
                    r = subprocess.run([str(CLI), "match", str(d / "db.mxy")] + paths + ["--format", fmt] + flags, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
                    arms[arm].append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr[-2000:]
            for arm, v in arms.items():
                out("  %-8s %-10s median %.3f  min %.3f  max %.3f  (n = %d)" % (fmt, arm, statistics.median(v), min(v), max(v), len(v)))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pass,cli")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--files", type=int, default=4096)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    if "pass" in a.parts:
        part_pass(a.reps, out)
    if "cli" in a.parts:
        part_cli(a.reps, a.files, out)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
