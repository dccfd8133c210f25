"""What the hit tally (csrc/tally.hip) costs and what it replaces, on the benchmark's batches: the headline batch (BASELINE configs[1]:
config c2, 10 M nginx lines) and the CIDR-heavy batch (configs[4]: c5), both from the synthetic generators under tools/.

Per batch, the step time of matchy_scanner_scan_device on the device-resident batch (wall clock around the call, which returns with
the results in host memory):

  off        tally off, counters only (fetch mode 0)
  on         tally on, counters only: the same plus k_tally_claim / k_tally_publish over the batch's records
  records    tally off, hit records moved to host memory (fetch mode 1 | 8, the benchmark's default) — what a host-side
             `sort | uniq -c` would need and the tally replaces
  top20      one read-out of the 20 most frequent values behind the `on` steps

and, from the MATCHY_AMD_TRACE lines of a few more `on` steps in a child process (the variable is read when a scanner is created),
the device time of the claim and the publish kernel alone (HIP events; the first step of a fresh tally publishes every value, the
later ones find them published).

    python tools/tally_timing.py [--lines N] [--steps K] [--warmup W] [--configs c2,c5] [--out profiles/tally_timing.txt]

The arms alternate step by step, so drift hits all of them; median, minimum and maximum are reported. --bench FILE ... appends the
JSON lines of bench.py runs (this tree and the parent commit, measured in the same session) under the figures."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

TRACE = re.compile(r"tally: (\d+) records, (\d+) distinct \(\+(\d+)\), rehashes=(\d+) pool_regrows=(\d+) direct_adds=(\d+), claim ([\d.]+) ms publish ([\d.]+) ms total ([\d.]+) ms")


def batch(config, lines):
    """(database blob, torch uint8 tensor with the batch on the device, bytes)"""
    import torch
    from tools import synth
    cfg = synth.config(config)
    blob = synth.build_db(cfg)
    cap = lines * 200 + (1 << 20)
    host = torch.empty(cap, dtype=torch.uint8)
    nbytes = synth.make_log_into(cfg, 0, lines, host.data_ptr(), cap, "nginx", 0)
    if nbytes > cap:
        raise SystemExit("batch larger than expected; lower --lines")
    dlog = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    dlog[:nbytes].copy_(host[:nbytes])
    torch.cuda.synchronize()
    return blob, dlog, nbytes


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": len(ms)}


def child(blob_path, config, lines, steps):
    """a few tally-on steps with the trace on; the lines go to stderr"""
    import torch
    import matchy_amd as M
    from tools import synth
    cfg = synth.config(config)
    cap = lines * 200 + (1 << 20)
    host = torch.empty(cap, dtype=torch.uint8)
    nbytes = synth.make_log_into(cfg, 0, lines, host.data_ptr(), cap, "nginx", 0)
    dlog = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    dlog[:nbytes].copy_(host[:nbytes])
    torch.cuda.synchronize()
    db = M.Database(Path(blob_path).read_bytes())
    sc = M.Scanner(db)
    sc.set_tally(True)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(steps):
        sc.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=0).close()
    sc.close()
    db.close()


def measure(config, lines, steps, warmup):
    import torch
    import matchy_amd as M
    blob, dlog, nbytes = batch(config, lines)
    db = M.Database(blob)
    stream = torch.cuda.current_stream().cuda_stream
    arms = {"off": (M.Scanner(db), 0), "on": (M.Scanner(db), 0), "records": (M.Scanner(db), 9)}
    arms["on"][0].set_tally(True)
    times = {k: [] for k in arms}
    hits = {}
    for it in range(warmup + steps):
        for k, (sc, mode) in arms.items():
            t0 = time.perf_counter()
            r = sc.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=mode)
            dt = (time.perf_counter() - t0) * 1e3
            hits[k] = r.n_hits
            r.close()
            if it >= warmup:
                times[k].append(dt)
    t0 = time.perf_counter()
    top = arms["on"][0].tally(20)
    top_ms = (time.perf_counter() - t0) * 1e3
    out = {"config": config, "lines": lines, "bytes": nbytes, "hits_per_batch": hits["off"], "distinct_values": top.distinct,
           "counted": top.matches, "counted_expected": hits["on"] * (warmup + steps),
           "step": {k: stats(v) for k, v in times.items()}, "top20_ms": round(top_ms, 3),
           "top3": [[t.decode("latin-1"), typ, n] for t, typ, n in list(top)[:3]]}
    for k in ("off", "on", "records"):
        out["step"][k]["GB_per_s"] = round(nbytes / (out["step"][k]["median_ms"] * 1e-3) / 1e9, 1)
    if top.matches != out["counted_expected"] or len({hits[k] for k in hits}) != 1:
        raise RuntimeError(f"tally counted {top.matches}, the scans reported {out['counted_expected']} ({hits})")
    for sc, _ in arms.values():
        sc.close()
    db.close()
    del dlog
    torch.cuda.empty_cache()
    # the kernels alone: a child with the trace on
    with tempfile.TemporaryDirectory() as d:
        p = Path(d) / "db.mxy"
        p.write_bytes(blob)
        env = dict(os.environ, MATCHY_AMD_TRACE="1")
        c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", str(p), "--configs", config, "--lines", str(lines), "--steps", "4"],
                           env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=900)
        if c.returncode != 0:
            raise RuntimeError(c.stderr.decode()[-2000:])
        rows = TRACE.findall(c.stderr.decode())
    out["kernels"] = [{"records": int(r[0]), "new_entries": int(r[2]), "rehashes": int(r[3]), "pool_regrows": int(r[4]), "direct_adds": int(r[5]),
                       "claim_ms": float(r[6]), "publish_ms": float(r[7]), "total_ms": float(r[8])} for r in rows]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench", nargs="*", default=[], help="LABEL=FILE pairs: files with bench.py JSON result lines to append")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.configs, args.lines, args.steps)
        return
    import matchy_amd.build as B
    B.build()
    out = {"batches": [measure(c, args.lines, args.steps, args.warmup) for c in args.configs.split(",")]}
    bench = {}
    for pair in args.bench:
        label, _, path = pair.partition("=")
        vals = []
        for ln in Path(path).read_text().splitlines():
            if ln.startswith("{"):
                j = json.loads(ln)
                vals.append({"value": j.get("value"), "unit": j.get("unit"), "step_ms": j.get("step_ms")})
        bench[label] = vals
    if bench:
        out["bench_py"] = bench
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
