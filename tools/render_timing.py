"""What rendering the records of a scan on the GPU (csrc/render.hip) costs next to the host renderer.

One batch of --lines nginx lines (tools/synth, config c2) resident in device memory, two databases: the headline's (c2: about one line
in twenty hits) and "dense", a database of all 255 /8 networks under which every line hits (standing in for the C5 batch, whose
ten-million-entry database is not built here). Per database and per flag set (no line keys; "line_number" + "input_line") the arms
alternate repetition by repetition in one process:
  (A) the scan, fetch mode 1, then the host renderer on its result (matchy_scan_result_to_ndjson / _lines, its four threads and its
      payload cache warm): wall clock of the scan call, wall clock of the renderer call;
  (B) the same scan armed with set_render: wall clock of the scan call (the text is in pinned memory when it returns), and the
      device times of matchy_scanner_get_render_timing: measure + offsets, write, the block's device-to-host copy.
Medians; the first armed scan of a scanner (which renders the payloads and repeats the pass) is not among the repetitions. Every
repetition compares the two texts byte for byte.

    python tools/render_timing.py [--reps R] [--lines N] [--out FILE]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lines", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import matchy_amd as M
    from tools import synth
    sink = open(args.out, "w") if args.out else None

    def out(s):
        print(s, flush=True)
        if sink:
            sink.write(s + "\n")
            sink.flush()

    cfg = synth.config("c2")
    text = synth.make_log(cfg, 0, args.lines)
    dense = M.DatabaseBuilder(build_epoch=1)
    for a in range(1, 256):
        dense.add_entry("%d.0.0.0/8" % a, {"k": "any"})
    blobs = (("headline", synth.build_db(cfg)), ("dense", dense.build()))
    dense.close()
    dlog = torch.empty(len(text) + 64, dtype=torch.uint8, device="cuda")
    dlog[:len(text)].copy_(torch.frombuffer(bytearray(text), dtype=torch.uint8))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ms = lambda t0: (time.perf_counter() - t0) * 1e3
    out("%d lines, %d bytes; milliseconds, median of %d" % (args.lines, len(text), args.reps))
    out("%9s %6s %10s %12s | %9s %9s %9s | %9s %8s %8s %8s" % ("database", "keys", "records", "text bytes", "A scan", "A render", "A sum", "B scan", "measure", "write", "d2h"))
    for name, blob in blobs:
        db = M.Database(blob)
        sc = M.Scanner(db, profile=True)
        for flags in (0, 3):
            sc.set_line_context(flags != 0)

            def host(res):
                return res.ndjson_text(text, source="x.log") if not flags else res.ndjson_lines_text(text, source="x.log", with_input_line=True)

            def scan(arm):
                if arm:
                    sc.set_render(flags=flags, source="x.log")
                t0 = time.perf_counter()
                res = sc.scan_device(dlog.data_ptr(), len(text), stream=stream, fetch_mode=1)
                return res, ms(t0)
            res, _ = scan(True)   # the payloads, the growth of the block and of the host renderer's cache
            host(res)
            res.close()
            a_scan, a_render, b_scan, dev = [], [], [], []
            n_records = n_bytes = 0
            for _ in range(args.reps):
                res, t = scan(False)
                t0 = time.perf_counter()
                want = host(res)
                a_render.append(ms(t0))
                a_scan.append(t)
                res.close()
                res, t = scan(True)
                got = res.rendered_ndjson()   # one copy out of pinned memory into a Python object: not part of either arm
                b_scan.append(t)
                tm = sc.render_timing_ms()
                dev.append((tm["measure"], tm["write"], tm["d2h"]))
                assert sc.render_counters()["rounds"] == 0
                assert sorted(got.split(b"\n")) == sorted(want.split(b"\n")), "the two renderers differ"   # two scans: device order may differ
                n_records, n_bytes = res.n_hits, len(got)
                res.close()
            med = statistics.median
            out("%9s %6s %10d %12d | %9.2f %9.2f %9.2f | %9.2f %8.3f %8.3f %8.3f" % (
                name, "lines" if flags else "none", n_records, n_bytes, med(a_scan), med(a_render), med(a_scan) + med(a_render), med(b_scan),
                med([d[0] for d in dev]), med([d[1] for d in dev]), med([d[2] for d in dev])))
        sc.close()
        db.close()


if __name__ == "__main__":
    main()
