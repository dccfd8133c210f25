"""`matchy extract` end to end with and without --render-on-gpu (csrc/extract_render.hip), on the benchmark's nginx log (BASELINE
configs[1]: config c2, 10 M lines), output to /dev/null, for --format json and --format text:

  (a) wall time of `matchy extract LOG --format F > /dev/null` with a command line built from the parent commit
      (--parent-cli PATH: a tree of that commit built elsewhere; without it (a) is reported as "unmeasured")
  (b) the same command from this tree, without the flag
  (c) the same command from this tree with --render-on-gpu
  (d) per batch, the device time of the pass's steps (HIP events: keys + sort, measure, write, copy of the block) beside the extraction
      kernels' of the same batch, from the MATCHY_AMD_TRACE lines of one more run of (c)

    python tools/extract_render_timing.py [--lines N] [--reps R] [--parent-cli PATH] [--out FILE]

Every command runs once unmeasured first (file cache, GPU clocks, code objects), then R times; the median and all values are reported,
the commands alternating so that drift hits all of them. What the record has to show: (b) against (a) within the spread of (a)'s own
repeats, and (c) against (b)."""
import argparse
import json
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def run(cli, log, fmt, extra=(), env=None):
    t0 = time.perf_counter()
    p = subprocess.run([cli, "extract", log, "--format", fmt, "--stats", *extra], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(p.stderr.decode()[-2000:])
    print("%s --format %s %s: %.3f s" % (cli, fmt, " ".join(extra), dt), file=sys.stderr, flush=True)
    return dt, p.stderr.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes
    import os
    import matchy_amd.build as B
    from tools import synth
    B.build()
    cfg = synth.config(args.config)
    cap = args.lines * 200 + (1 << 20)
    buf = ctypes.create_string_buffer(cap)
    nbytes = synth.make_log_into(cfg, 0, args.lines, ctypes.addressof(buf), cap, "nginx", 0)
    out = {"lines": args.lines, "config": args.config, "bytes": nbytes, "formats": {}}
    with tempfile.TemporaryDirectory() as d:
        log = str(Path(d) / "nginx.log")
        with open(log, "wb") as f:
            f.write(memoryview(buf)[:nbytes])
        del buf
        runs = {"b_this_tree": (str(B.CLI), ()), "c_render_on_gpu": (str(B.CLI), ("--render-on-gpu",))}
        if args.parent_cli:
            runs = {"a_parent": (args.parent_cli, ()), **runs}
        for fmt in ("json", "text"):
            res = {}
            times = {k: [] for k in runs}
            found = {}
            for k, (cli, extra) in runs.items():
                run(cli, log, fmt, extra)   # unmeasured
            for _ in range(args.reps):
                for k, (cli, extra) in runs.items():
                    dt, err = run(cli, log, fmt, extra)
                    times[k].append(round(dt, 3))
                    m = re.search(r"Patterns found: ([\d,]+)", err)
                    found[k] = int(m.group(1).replace(",", "")) if m else None
            for k in runs:
                res[k] = {"seconds_median": statistics.median(times[k]), "seconds": times[k], "values_printed": found[k]}
            if not args.parent_cli:
                res["a_parent"] = "unmeasured"
            if len(set(found.values())) != 1:
                raise RuntimeError(f"the command lines print different numbers of values: {found}")
            env = dict(os.environ, MATCHY_AMD_TRACE="1")
            _, err = run(str(B.CLI), log, fmt, ("--render-on-gpu",), env)
            rows = re.findall(r"extract text: (\d+) records, block of (\d+) bytes, status (\d+); keys \+ sort ([\d.]+) ms, measure ([\d.]+) ms, write ([\d.]+) ms, "
                              r"copy ([\d.]+) ms, behind ([\d.]+) ms", err)
            res["d_batches"] = [{"records": int(r[0]), "block_bytes": int(r[1]), "status": int(r[2]), "keys_sort_ms": float(r[3]), "measure_ms": float(r[4]),
                                 "write_ms": float(r[5]), "copy_ms": float(r[6]), "extraction_kernels_ms": float(r[7])} for r in rows]
            if rows:
                for name in ("keys_sort_ms", "measure_ms", "write_ms", "copy_ms", "extraction_kernels_ms"):
                    res["d_%s_total" % name] = round(sum(b[name] for b in res["d_batches"]), 3)
                res["d_records_total"] = sum(b["records"] for b in res["d_batches"])
            out["formats"][fmt] = res
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
