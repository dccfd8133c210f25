"""What `matchy match --gz-on-gpu --gz-members` buys on ONE large multi-member .gz file, on the headline log shape (tools/synth: config c2,
nginx lines). Three files of the same 256 MiB of text:

  (a) bgzf   BGZF-style members of 64 KiB of text, cut at arbitrary bytes, the empty block last
  (b) 1mib   members of 1 MiB of text
  (c) one    one member: the control — it has no members to split and must go to the host in both arms

  pass   (a) and (b) through matchy_scanner_scan_gz_files, counts only: device time of k_gz_inflate and of k_gz_file_verdict + k_gz_seal_files
         from matchy_scanner_get_gz_timing, GB/s of inflated text, the scan's own device time beside them. (c) is not timed here: one
         wave on 256 MiB takes about half a minute per repetition (profiles/gz_inflate_timing.txt: 1.77 s for 16 MiB).
  cli    `--format summary` wall clock of the process per file, page cache warm: arm A = this tree WITHOUT the flags (the gzread path
         of read_input), arm B = --gz-on-gpu --gz-members. The arms alternate repetition by repetition; median, minimum, maximum.
         --batch-bytes is 320 MiB in both arms: a file must fit one pack, text and separator.

The text is 16 MiB of the log repeated 16 times, so that every distinct member is compressed once (level 6).

    python tools/gz_members_timing.py [--parts pass,cli] [--reps R] [--mib N] [--out FILE]"""
import argparse
import json
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CLI = ROOT / "matchy_amd" / "bin" / "matchy"
BATCH = 320 << 20


def headline(nbytes):
    from tools import synth
    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, max(100, nbytes // 100))
    assert len(text) >= nbytes, "raise the line estimate"
    return synth.build_db(cfg), text[:nbytes - 1] + b"\n"


def member(text, bgzf):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = c.compress(text) + c.flush()
    head = bytes([0x1F, 0x8B, 8, 4 if bgzf else 0, 0, 0, 0, 0, 0, 3])
    if bgzf:
        head += struct.pack("<H", 6) + b"BC\x02\x00" + struct.pack("<H", 18 + len(body) + 8 - 1)
    return head + body + struct.pack("<II", zlib.crc32(text), len(text))


def build_files(unit, repeats):
    """{name: (file, members)} of unit * repeats"""
    out = {}
    for name, block, bgzf in (("bgzf", 1 << 16, True), ("1mib", 1 << 20, False)):
        one = b"".join(member(unit[i:i + block], bgzf) for i in range(0, len(unit), block))
        n = -(-len(unit) // block) * repeats
        out[name] = (one * repeats + (member(b"", True) if bgzf else b""), n + (1 if bgzf else 0))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body, crc = b"", 0
    for _ in range(repeats):
        body += c.compress(unit)
        crc = zlib.crc32(unit, crc)
    body += c.flush()
    out["one"] = (bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3]) + body + struct.pack("<II", crc, len(unit) * repeats & 0xFFFFFFFF), 1)
    return out


def part_pass(blob, files, text_len, reps, out):
    import matchy_amd as M
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    out("pass: device milliseconds, median of %d (inflate includes the CRC; verdict+seal = k_gz_file_verdict + k_gz_seal_files; scan = the scan's own total)" % reps)
    out("%6s %8s %10s %10s %13s %9s %9s %9s" % ("file", "members", "packed", "inflate", "verdict+seal", "scan", "GB/s", "hits"))
    for name in ("bgzf", "1mib"):
        data, n = files[name]
        ms = []
        for _ in range(reps):
            r = sc.scan_gz_files([data], fetch_mode=0)
            assert r.gz_file_status() == [0] and len(r.gz_status()) == n, "the file failed"
            t, hits = sc.gz_timing_ms(), r.n_hits
            ms.append((t["inflate"], t["seal"], sc.timing_ms()["total"]))
            r.close()
        inflate, seal, scan = (statistics.median(v) for v in zip(*ms))
        out("%6s %8d %10d %10.3f %13.3f %9.3f %9.3f %9d" % (name, n, len(data), inflate, seal, scan, text_len / (inflate + seal) / 1e6, hits))
    out("%6s %8d %10d   not measured: one wave, about %d s per repetition at the one-wave rate on file" % ("one", 1, len(files["one"][0]), round(text_len / (16 << 20) * 1.77)))
    sc.close(); db.close()


def part_cli(blob, files, text_len, reps, out):
    d = Path(tempfile.mkdtemp(prefix="gz_members_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        out("cli: one .gz file of %d bytes of text per run, --format summary, --batch-bytes %d, wall clock seconds of the process" % (text_len, BATCH))
        out("     arm A = this tree without the flags (gzread on the reader thread), arm B = --gz-on-gpu --gz-members")
        for name in ("bgzf", "1mib", "one"):
            p = d / (name + ".log.gz")
            p.write_bytes(files[name][0])
            arms = {"A gzread": [], "B gz-members": []}
            where = ""
            for _ in range(reps):
                for arm, flags in (("A gzread", []), ("B gz-members", ["--gz-on-gpu", "--gz-members"])):
                    t0 = time.perf_counter()
                    r = subprocess.run([str(CLI), "match", str(d / "db.mxy"), str(p), "--format", "summary", "-s", "--batch-bytes", str(BATCH)] + flags,
                                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
                    arms[arm].append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr[-2000:]
                    if flags:
                        m = re.search(rb"Inflated (\d+) \.gz inputs on the GPU.*, (\d+) read on the host\n.*gz members on the GPU: (\d+) in (\d+)", r.stderr)
                        where = "on the GPU: %s file(s), %s members; on the host after a verdict: %s" % (m.group(1).decode(), m.group(3).decode(), m.group(2).decode()) if m else "?"
            for arm, v in arms.items():
                out("  %-5s %-13s median %.3f  min %.3f  max %.3f  (n = %d)" % (name, arm, statistics.median(v), min(v), max(v), len(v)))
            out("  %-5s arm B: %s" % (name, where))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pass,cli")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mib", type=int, default=256, help="MiB of text per file (a multiple of 16)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    blob, unit = headline(16 << 20)
    repeats = max(1, a.mib // 16)
    files = build_files(unit, repeats)
    text_len = len(unit) * repeats
    out("files: %d bytes of text each; compressed: bgzf %d (%d members), 1mib %d (%d members), one %d" %
        (text_len, len(files["bgzf"][0]), files["bgzf"][1], len(files["1mib"][0]), files["1mib"][1], len(files["one"][0])))
    if "pass" in a.parts:
        part_pass(blob, files, text_len, a.reps, out)
    if "cli" in a.parts:
        part_cli(blob, files, text_len, a.reps, out)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")
    json.dump({"ok": True}, sys.stdout)
    print()


if __name__ == "__main__":
    main()
