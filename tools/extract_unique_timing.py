"""`matchy extract --unique` before and after the device set of distinct texts (csrc/distinct.hip), on the benchmark's nginx log
(BASELINE configs[1]: config c2, 10 M lines):

  (a) wall time of `matchy extract LOG --unique --format text > /dev/null` with a command line built from the parent commit
      (--parent-cli PATH: a tree of that commit built elsewhere; without it (a) is reported as "unmeasured")
  (b) the same command from this tree
  (c) per batch, the device time of the dedup kernels (HIP events around k_distinct_claim .. k_distinct_publish, growth included)
      beside the extraction kernels' of the same batch, from the MATCHY_AMD_TRACE lines of one more run of (b)

    python tools/extract_unique_timing.py [--lines N] [--reps R] [--parent-cli PATH] [--out FILE]

Every command runs once unmeasured first (file cache, GPU clocks, code objects), then R times; the median and all values are reported,
(a) and (b) alternating so that drift hits both."""
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


def run(cli, log, env=None):
    t0 = time.perf_counter()
    p = subprocess.run([cli, "extract", log, "--unique", "--format", "text", "--stats"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(p.stderr.decode()[-2000:])
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
    out = {"lines": args.lines, "config": args.config, "bytes": nbytes}
    with tempfile.TemporaryDirectory() as d:
        log = str(Path(d) / "nginx.log")
        with open(log, "wb") as f:
            f.write(memoryview(buf)[:nbytes])
        del buf
        clis = {"b_this_tree": str(B.CLI)}
        if args.parent_cli:
            clis["a_parent"] = args.parent_cli
        times = {k: [] for k in clis}
        found = {}
        for k, cli in clis.items():
            run(cli, log)   # unmeasured
        for _ in range(args.reps):
            for k, cli in clis.items():
                dt, err = run(cli, log)
                times[k].append(round(dt, 3))
                m = re.search(r"Patterns found: ([\d,]+)", err)
                found[k] = int(m.group(1).replace(",", "")) if m else None
        for k in clis:
            out[k] = {"seconds_median": statistics.median(times[k]), "seconds": times[k], "values_printed": found[k]}
        if not args.parent_cli:
            out["a_parent"] = "unmeasured"
        elif found["a_parent"] != found["b_this_tree"]:
            raise RuntimeError(f"the two command lines print different numbers of values: {found}")
        env = dict(os.environ, MATCHY_AMD_TRACE="1")
        _, err = run(str(B.CLI), log, env)
        rows = [(int(a), int(b), float(c), float(e)) for a, b, c, e in
                re.findall(r"distinct: (\d+) of (\d+) candidates are new, dedup ([\d.]+) ms behind ([\d.]+) ms", err)]
        out["c_batches"] = [{"new": a, "candidates": b, "dedup_ms": c, "extraction_kernels_ms": e} for a, b, c, e in rows]
        if rows:
            out["c_dedup_ms_total"] = round(sum(r[2] for r in rows), 3)
            out["c_extraction_kernels_ms_total"] = round(sum(r[3] for r in rows), 3)
            out["c_candidates_total"] = sum(r[1] for r in rows)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
