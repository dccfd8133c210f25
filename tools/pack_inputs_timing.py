"""What segmented scans (csrc/segments.hip) and `matchy match --pack-inputs` buy for many small inputs, and what the pass costs, on the
benchmark's log shapes (tools/synth: config c2, nginx lines — the headline — and c5, the CIDR-heavy one).

  library      N segments of ~64 KiB of the headline log (cut at line ends): N calls of matchy_scanner_scan, one per segment, against
               the same bytes as packed batches of --batch-mib with matchy_scanner_set_segments. Wall clock around all calls of an arm.
  cli          the same segments as N files: `matchy match --format summary` and the default JSON, with and without --pack-inputs.
               Wall clock of the process.
  pass         one device-resident batch of --lines lines with 1, 1 024 and 65 536 segments against the same scan without segments:
               step time of matchy_scanner_scan_device (wall clock around the call, fetch mode 0 for c2, 1 | 8 — the records cross the
               bus — for c5), line context off and on, and the HIP-event times of the three passes from a profiling scanner.

    python tools/pack_inputs_timing.py [--parts library,cli,pass] [--segments N] [--lines N] [--reps R] [--steps K] [--out FILE]

The arms of a comparison alternate repetition by repetition, so drift hits all of them; median, minimum and maximum are reported.
--bench LABEL=FILE ... appends the JSON lines of bench.py runs (this tree and the parent commit, measured in the same session)."""
import argparse
import ctypes
import json
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


def host_log(config, lines):
    """(database blob, pinned-size torch uint8 tensor on the host, bytes)"""
    import torch
    from tools import synth
    cfg = synth.config(config)
    blob = synth.build_db(cfg)
    cap = lines * 200 + (1 << 20)
    host = torch.empty(cap, dtype=torch.uint8)
    nbytes = synth.make_log_into(cfg, 0, lines, host.data_ptr(), cap, "nginx", 0)
    if nbytes > cap:
        raise SystemExit("log larger than expected; lower the line count")
    return blob, host, nbytes


def cut_points(view, nbytes, targets):
    """for every target offset the start of the next line (0 stays 0), increasing; targets behind the last '\\n' are dropped"""
    out = []
    for t in targets:
        if t == 0:
            p = 0
        else:
            q = view.find(b"\n", t - 1, nbytes)
            if q < 0 or q + 1 >= nbytes:
                break
            p = q + 1
        if not out or p > out[-1]:
            out.append(p)
    return out


def stats(v, unit="s"):
    return {f"median_{unit}": round(statistics.median(v), 4), f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4), "n": len(v)}


# ------------------------------------------------------------------------------------------------ library
def part_library(n_segments, seg_bytes, batch_bytes, reps):
    import matchy_amd as M
    lines = max(1000, n_segments * seg_bytes // 120)
    blob, host, nbytes = host_log("c2", lines)
    view = host.numpy()[:nbytes].tobytes()
    starts = cut_points(view, nbytes, range(0, min(nbytes, n_segments * seg_bytes), seg_bytes))[:n_segments]
    end = starts[-1] + seg_bytes if len(starts) == n_segments else nbytes
    end = min(nbytes, (view.find(b"\n", end - 1) + 1) or nbytes)
    ends = starts[1:] + [end]
    # packs: consecutive segments while the pack stays within batch_bytes
    packs, first = [], 0
    for i in range(1, len(starts) + 1):
        if i == len(starts) or ends[i] - starts[first] > batch_bytes:
            packs.append((first, i))
            first = i
    base = host.data_ptr()
    db = M.Database(blob)
    single, packed = M.Scanner(db), M.Scanner(db)
    times = {"one_scan_per_segment": [], "packed_with_segments": []}
    hits = {}
    for rep in range(reps + 1):   # the first repetition warms both arms up
        t0 = time.perf_counter()
        n = 0
        for s, e in zip(starts, ends):
            r = single.scan_ptr(base + s, e - s)
            n += r.n_hits
            r.close()
        t_single = time.perf_counter() - t0
        t0 = time.perf_counter()
        m, per_segment = 0, 0
        for a, b in packs:
            packed.set_segments([s - starts[a] for s in starts[a:b]])
            r = packed.scan_ptr(base + starts[a], ends[b - 1] - starts[a])
            m += r.n_hits
            per_segment += sum(s["hits"] for s in r.segments)
            r.close()
        t_packed = time.perf_counter() - t0
        hits = {"one_scan_per_segment": n, "packed_with_segments": m, "sum_of_segment_tables": per_segment}
        if rep:
            times["one_scan_per_segment"].append(t_single)
            times["packed_with_segments"].append(t_packed)
    if len(set(hits.values())) != 1:
        raise RuntimeError(f"the arms disagree: {hits}")
    single.close(); packed.close(); db.close()
    total = end - starts[0]
    out = {"segments": len(starts), "bytes": total, "packs": len(packs), "batch_bytes": batch_bytes, "hits": hits["packed_with_segments"],
           "wall": {k: stats(v) for k, v in times.items()}}
    for k, v in out["wall"].items():
        v["GB_per_s"] = round(total / v["median_s"] / 1e9, 2)
        v["us_per_segment"] = round(v["median_s"] / len(starts) * 1e6, 1)
    return out, (blob, view, starts, ends)


# ------------------------------------------------------------------------------------------------ command line
def part_cli(blob, view, starts, ends, reps, batch_mib):
    d = Path(tempfile.mkdtemp(prefix="pack_timing_"))
    try:
        (d / "db.mxy").write_bytes(blob)
        names = []
        for i, (s, e) in enumerate(zip(starts, ends)):
            names.append("%05d.log" % i)
            (d / names[-1]).write_bytes(view[s:e])
        arms = {"summary": ["--format", "summary"], "summary_packed": ["--format", "summary", "--pack-inputs"], "json": [], "json_packed": ["--pack-inputs"]}
        times, sizes = {k: [] for k in arms}, {}
        for rep in range(reps + 1):
            for k, flags in arms.items():
                t0 = time.perf_counter()
                p = subprocess.run([str(CLI), "match", "db.mxy"] + names + ["--batch-bytes", str(batch_mib << 20)] + flags, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
                dt = time.perf_counter() - t0
                if p.returncode != 0:
                    raise RuntimeError(p.stderr.decode()[-2000:])
                sizes[k] = len(p.stdout)
                if rep:
                    times[k].append(dt)
        if sizes["json"] != sizes["json_packed"] or sizes["summary"] or sizes["summary_packed"]:
            raise RuntimeError(f"the arms print different amounts: {sizes}")
        return {"files": len(names), "stdout_bytes": sizes["json"], "wall": {k: stats(v) for k, v in times.items()}}
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ------------------------------------------------------------------------------------------------ cost of the pass
def part_pass(config, lines, steps, warmup, mode):
    import torch
    import matchy_amd as M
    blob, host, nbytes = host_log(config, lines)
    view = host.numpy()[:nbytes].tobytes()
    dlog = torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda:0")
    dlog[:nbytes].copy_(host[:nbytes])
    torch.cuda.synchronize()
    tables = {n: cut_points(view, nbytes, [i * (nbytes // n) for i in range(n)]) for n in (1, 1024, 65536)}
    del view
    db = M.Database(blob)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"config": config, "lines": lines, "bytes": nbytes, "fetch_mode": mode}
    for line_ctx in (False, True):
        arms = {"none": None, **{str(len(t)): t for t in tables.values()}}
        scanners = {k: M.Scanner(db) for k in arms}
        carr = {k: (ctypes.c_uint32 * len(t))(*t) for k, t in arms.items() if t is not None}
        L = M.lib()
        for sc in scanners.values():
            sc.set_line_context(line_ctx)
        times, hits = {k: [] for k in arms}, {}
        for it in range(warmup + steps):
            for k, table in arms.items():
                sc = scanners[k]
                t0 = time.perf_counter()
                if table is not None:   # the C call alone: the table as a ctypes array is built once, outside the timed region
                    L.matchy_scanner_set_segments(sc._h, carr[k], len(table))
                r = sc.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=mode)
                dt = (time.perf_counter() - t0) * 1e3
                hits[k] = r.n_hits
                if table is not None and sum(s["hits"] for s in r.segments) != r.n_hits:
                    raise RuntimeError("the segment table does not add up")
                r.close()
                if it >= warmup:
                    times[k].append(dt)
        if len(set(hits.values())) != 1:
            raise RuntimeError(f"the arms disagree: {hits}")
        for sc in scanners.values():
            sc.close()
        # the kernels alone: a profiling scanner (HIP events around the three passes)
        kernels = {}
        prof = M.Scanner(db, profile=True)
        prof.set_line_context(line_ctx)
        for k, table in arms.items():
            if table is None:
                continue
            rows = []
            for _ in range(4):
                prof.set_segments(table)
                prof.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=mode).close()
                rows.append(prof.segment_timing_ms())
            kernels[k] = {name: round(statistics.median(r[name] for r in rows[1:]), 4) for name in ("build", "records", "lines")}
        prof.close()
        out["line_context_on" if line_ctx else "line_context_off"] = {"records": hits["none"], "step": {k: stats(v, "ms") for k, v in times.items()}, "kernels_ms": kernels}
    db.close()
    del dlog
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="library,cli,pass")
    ap.add_argument("--segments", type=int, default=20000)
    ap.add_argument("--segment-kib", type=int, default=64)
    ap.add_argument("--batch-mib", type=int, default=256)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pack_inputs_timing.txt"))
    ap.add_argument("--bench", nargs="*", default=[], help="LABEL=FILE pairs: files with bench.py JSON result lines to append")
    args = ap.parse_args()
    import matchy_amd.build as B
    B.build()
    parts = args.parts.split(",")
    out = {}
    if "library" in parts or "cli" in parts:
        lib, data = part_library(args.segments, args.segment_kib << 10, args.batch_mib << 20, args.reps)
        print("library:", json.dumps(lib), file=sys.stderr, flush=True)
        if "library" in parts:
            out["library"] = lib
        if "cli" in parts:
            out["command_line"] = part_cli(*data, args.reps, args.batch_mib)
            print("command line:", json.dumps(out["command_line"]), file=sys.stderr, flush=True)
        del data
    if "pass" in parts:
        out["pass"] = []
        for config, mode in (("c2", 0), ("c5", 9)):
            out["pass"].append(part_pass(config, args.lines, args.steps, args.warmup, mode))
            print("pass:", json.dumps(out["pass"][-1]), file=sys.stderr, flush=True)
    bench = {}
    for pair in args.bench:
        label, _, path = pair.partition("=")
        vals = []
        for ln in Path(path).read_text().splitlines():
            if ln.startswith("{"):
                j = json.loads(ln)
                vals.append({"value": j.get("value"), "unit": j.get("unit"), "ms_per_step": j.get("ms_per_step")})
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
