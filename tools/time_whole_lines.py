"""What whole-line mode (csrc/whole_lines.hip) does with a list of values, and what answered such a list before it.

Input: a synthetic list from the generators under tools/ — by default 10 M queries, 70 % IPv4 addresses, 25 % names, 5 % SHA-256
hashes, 2 % of them keys of the database (BASELINE configs[1]: config c2, 100 K mixed indicators) — resident in device memory. The
list is a block of --unique distinct lines (default 1 M) repeated to the wanted length: a query costs the same the second time (the
mode keeps no cache).

Reported:
  step            wall clock around matchy_scanner_scan_device (counters only), median / min / max, queries per second, GB/s
  intervals       HIP-event times of the mode (matchy_scanner_get_whole_lines_timing): count + prefix, scatter + classify, lookups
  line_count_ms   the streaming '\\n' count kernel of line_index.hip over the same bytes (a scan with line context): the yardstick for
                  the front end, which is two such passes and a kernel over the lines
  host_loop       tools/query_loop.cpp — a loop over matchy_query, the only way to answer such a list without the mode — on 1 and on
                  16 host threads over the first --host-queries lines, in the same run on the same machine

    python tools/time_whole_lines.py [--queries N] [--unique N] [--steps K] [--warmup W] [--host-queries N] [--out profiles/whole_lines.txt]"""
import argparse
import json
import random
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_block(cfg, n, seed=20261020):
    """n distinct-ish query lines: 70 % IPv4, 25 % names, 5 % hashes; 2 % are keys of the database"""
    from tools import synth
    keys = {"ip": [], "name": [], "hash": []}
    for key, _ in synth.ioc_entries(cfg):
        k = key.decode()
        if "/" in k or "*" in k:
            continue
        if k.replace(".", "").isdigit():
            keys["ip"].append(k)
        elif len(k) in (32, 40, 64) and all(c in "0123456789abcdefABCDEF" for c in k):
            keys["hash"].append(k)
        elif "." in k:
            keys["name"].append(k)
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        u = rng.random()
        kind = "ip" if u < 0.70 else "name" if u < 0.95 else "hash"
        if rng.random() < 0.02 and keys[kind]:
            out.append(rng.choice(keys[kind]))
        elif kind == "ip":
            out.append("%d.%d.%d.%d" % (rng.randrange(1, 224), rng.randrange(256), rng.randrange(256), rng.randrange(256)))
        elif kind == "name":
            out.append("h%d.site-%d.example-%d.net" % (rng.randrange(100000), rng.randrange(5000), rng.randrange(1000)))
        else:
            out.append("%064x" % rng.getrandbits(256))
    return ("\n".join(out) + "\n").encode()


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": len(ms)}


def host_loop(blob, block, n_queries, threads_list):
    with tempfile.TemporaryDirectory() as d:
        d = Path(d)
        (d / "db.mxy").write_bytes(blob)
        lines = block.split(b"\n")[:-1]
        reps = (n_queries + len(lines) - 1) // len(lines)
        (d / "q.txt").write_bytes(b"\n".join((lines * reps)[:n_queries]) + b"\n")
        exe = d / "query_loop"
        lib = ROOT / "matchy_amd" / "lib"
        subprocess.run(["g++", "-O2", "-std=c++17", str(ROOT / "tools" / "query_loop.cpp"), "-I", str(ROOT / "include"), "-L", str(lib), "-lmatchy_amd",
                        "-lpthread", "-Wl,-rpath," + str(lib), "-o", str(exe)], check=True)
        out = []
        for t in threads_list:
            p = subprocess.run([str(exe), str(d / "db.mxy"), str(d / "q.txt"), str(t), "3"], capture_output=True, text=True, timeout=1800)
            if p.returncode != 0:
                raise RuntimeError(p.stderr[-2000:])
            out.append(json.loads(p.stdout))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--unique", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=2_000_000)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import matchy_amd as M
    import matchy_amd.build as B
    from tools import synth
    B.build()
    cfg = synth.config(args.config)
    blob = synth.build_db(cfg)
    unique = min(args.unique, args.queries)
    block = make_block(cfg, unique)
    reps = max(1, args.queries // unique)
    data = block * reps
    n_queries = unique * reps
    dlog = torch.empty(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    dlog[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    db = M.Database(blob)
    sc = M.Scanner(db, profile=True)
    sc.set_whole_lines(True)
    wall, parts = [], {"count_prefix": [], "scatter_classify": [], "lookup": []}
    hits = None
    for it in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        r = sc.scan_device(dlog.data_ptr(), len(data), stream=stream, fetch_mode=0)
        dt = (time.perf_counter() - t0) * 1e3
        hits = r.n_hits
        r.close()
        if it >= args.warmup:
            wall.append(dt)
            for k, v in sc.whole_lines_timing_ms().items():
                parts[k].append(v)
    counters = sc.whole_lines_counters()
    sc.close()
    yard = M.Scanner(db, profile=True)
    yard.set_line_context(True)
    count_ms = []
    for it in range(args.warmup + 5):
        yard.scan_device(dlog.data_ptr(), len(data), stream=stream, fetch_mode=0).close()
        if it >= args.warmup:
            count_ms.append(yard.line_timing_ms()["count"])
    yard.close()
    db.close()
    step = stats(wall)
    step["queries_per_s"] = round(n_queries / (step["median_ms"] * 1e-3))
    step["GB_per_s"] = round(len(data) / (step["median_ms"] * 1e-3) / 1e9, 2)
    out = {"config": args.config, "queries": n_queries, "distinct_lines": unique, "bytes": len(data), "hits": hits, "counters": counters,
           "step": step, "intervals_ms": {k: round(statistics.median(v), 4) for k, v in parts.items()},
           "line_count_ms": round(statistics.median(count_ms), 4),
           "host_loop": host_loop(blob, block, min(args.host_queries, n_queries), (1, 16))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
