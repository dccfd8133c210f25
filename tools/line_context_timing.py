"""Cost of line context on the headline workload of bench.py (config c2, 10 M lines, one GPU, compact records):

  (a) step time with line context off      (b) step time with it on
  (c) the streaming '\\n' count kernel alone, against the device-to-device copy rate of a 1 GiB buffer (bench.py's measurement)
  (d) the host loop `matchy match` runs without --line-numbers (memchr over the gaps between hits) over the same batch, one thread

    python tools/line_context_timing.py [--lines N] [--steps K] [--warmup W] [--out FILE]

Steps are timed like bench.py times them: wall clock around scan_device (launch to results in host memory), batch resident in HBM."""
import argparse
import ctypes
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def gaps_lib():
    so = ROOT / "tools" / "libmemchr_gaps.so"
    src = ROOT / "tools" / "memchr_gaps.cpp"
    if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    L = ctypes.CDLL(str(so))
    L.memchr_gaps.restype = ctypes.c_uint64
    L.memchr_gaps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="off / on are timed alternately this many times: the spread of the rounds is the noise")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import matchy_amd as M
    from tools import synth

    cfg = synth.config(args.config)
    db = M.Database(synth.build_db(cfg))
    sc = M.Scanner(db, profile=True)
    cap = args.lines * 200 + (1 << 20)
    host = torch.empty(cap, dtype=torch.uint8)
    nbytes = synth.make_log_into(cfg, 0, args.lines, host.data_ptr(), cap, "nginx", 0)
    dev = torch.device("cuda", 0)
    dlog = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    dlog[:nbytes].copy_(host[:nbytes])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def steps(mode, n):
        ts, last = [], None
        for _ in range(n):
            t0 = time.perf_counter()
            r = sc.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=mode)
            ts.append((time.perf_counter() - t0) * 1e3)
            last = (r.lines, r.candidates, r.n_hits, r.lines_with_matches)
            r.close()
        return ts, last

    out = {"bytes": nbytes, "lines": args.lines, "config": args.config, "tile_bytes": M.LINE_TILE}
    for mode, name in ((9, "compact"), (4, "device")):
        rounds = {"off": [], "on": []}
        count_ms, prefix_ms, resolve_ms = [], [], []
        for _ in range(args.rounds):
            for on in (False, True):
                sc.set_line_context(on)
                steps(mode, args.warmup)
                ts, last = steps(mode, args.steps)
                rounds["on" if on else "off"].append(statistics.median(ts))
                if on:
                    lt = sc.line_timing_ms()
                    count_ms.append(lt["count"]); prefix_ms.append(lt["prefix"]); resolve_ms.append(lt["resolve"])
                    out[name + "_result"] = dict(newlines=last[0], hits=last[2], lines_with_matches=last[3])
        out[name] = {"step_off_ms_rounds": [round(x, 4) for x in rounds["off"]], "step_on_ms_rounds": [round(x, 4) for x in rounds["on"]],
                     "step_off_ms": round(statistics.median(rounds["off"]), 4), "step_on_ms": round(statistics.median(rounds["on"]), 4),
                     "k_line_count_ms": round(statistics.median(count_ms), 4), "prefix_ms": round(statistics.median(prefix_ms), 4),
                     "resolve_and_distinct_ms": round(statistics.median(resolve_ms), 4)}
    c = out["compact"]["k_line_count_ms"]
    out["k_line_count_GBps"] = round(nbytes / (c * 1e-3) / 1e9, 1) if c else None
    # the card's copy rate, as bench.py --full measures it (read + write bytes of a 1 GiB device-to-device copy)
    nb = 1 << 30
    a = torch.empty(nb, dtype=torch.uint8, device=dev); b = torch.empty(nb, dtype=torch.uint8, device=dev)
    a.fill_(1)
    for _ in range(2):
        b.copy_(a)
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        b.copy_(a)
    e1.record(); torch.cuda.synchronize()
    out["device_copy_GBps_read_plus_write"] = round(5 * 2 * nb / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
    del a, b
    # (d) the host loop over the same batch: hits in canonical order (fetch_mode 3), one thread
    sc.set_line_context(True)
    r = sc.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=3)
    n = r._raw.n_hits
    starts = np.frombuffer(ctypes.string_at(ctypes.cast(r._raw.hits, ctypes.c_void_p).value, n * 16), dtype="<u4").reshape(-1, 4)[:, 0].copy()
    want = r.lines_with_matches
    r.close()
    G = gaps_lib()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        got = G.memchr_gaps(host.data_ptr(), starts.ctypes.data, n)
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    assert got == want, (got, want)
    out["host_memchr_loop_ms"] = round(best, 3)
    out["host_memchr_loop_hits"] = int(n)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
