#!/usr/bin/env python3
"""bench.py — `matchy match` hot path on MI355X: log GB/s scanned (+ lines/s) at a 100K-indicator database.

Contract: python bench.py --gpus N --steps K --warmup W   (N>1: launched by torch.distributed.run, one rank per GPU).
A "step" is one pass of the hot path (tokenize -> rare validators -> database lookup -> hit records on the host)
over one batch of synthetic nginx log that is ALREADY RESIDENT IN HBM when the timed region starts.

Workload at N=1 = BASELINE.json configs[1]: 100K mixed IoCs (40K IPv4 + 10K CIDR + 35K domains + 15K hashes),
10M nginx-style lines, 1x MI355X. For N>1 every rank scans its own 10M-line block (line-block sharding, no
collective on the data path; `scaling` = weak). Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline (`value`, `ms_per_step` = one timed step).
`--full` adds every other leg (records left in HBM, batches in flight, the host-buffer entry, scatter / gather, the
measured copy peak, the CPU baselines and the same-run parity check). `--dump-outputs DIR` writes the last timed step's
hit records as .npy files, so that two builds can be compared output for output on identical input.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)


fetch_hits = 9
DUMP_LIMIT = 64 << 20   # --dump-outputs: bytes of .npy data at most


def hit_arrays(res):
    """The hit records of a host-resident ScanResult as float64 arrays in canonical order (the device order of fetch modes 1 / 9
    varies from run to run): hits (n, 6) = [start, end, item type, kind (0 ip, 1 pattern), prefix_len, ip_data_offset] and
    ids (m, 3) = [row of hits, pattern id, data offset]."""
    import numpy as np
    import matchy_amd as M
    types = {name: i for i, name in enumerate(M.ITEM_TYPE_NAMES)}
    recs = sorted(((h["start"], h["end"], types[h["type"]], 0 if h["kind"] == "ip" else 1, h["prefix_len"], h["ip_data_offset"],
                    tuple(h["ids"]), tuple(h["offs"])) for h in res.hits()))
    hits = np.array([r[:6] for r in recs], dtype=np.float64).reshape(-1, 6)
    ids = np.array([(i, pid, off) for i, r in enumerate(recs) for pid, off in zip(r[6], r[7])], dtype=np.float64).reshape(-1, 3)
    return hits, ids


def dump_outputs(out_dir, counts, hits, ids):
    """--dump-outputs: counts / hits / hit_ids as .npy files; hit rows beyond DUMP_LIMIT are thinned to a sample drawn with a fixed seed."""
    import numpy as np
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    row_bytes = hits.shape[1] * 8 + (ids.nbytes / max(1, len(hits)))
    if hits.nbytes + ids.nbytes > DUMP_LIMIT:
        keep = np.sort(np.random.default_rng(0).choice(len(hits), int(0.9 * DUMP_LIMIT / row_bytes), replace=False))
        new_row = np.full(len(hits), -1, dtype=np.int64)
        new_row[keep] = np.arange(len(keep))
        ids = ids[np.isin(ids[:, 0].astype(np.int64), keep)]
        ids[:, 0] = new_row[ids[:, 0].astype(np.int64)]
        hits = hits[keep]
    np.save(out / "counts.npy", np.array(counts, dtype=np.float64))
    np.save(out / "hits.npy", hits)
    np.save(out / "hit_ids.npy", ids)


def run_strong(args, rank, local_rank, world, rehearse, torch, dist, dev, coll_dev):
    """--scaling strong: ONE job (BASELINE configs[3]: 100 M lines of the C4 log by default) cut into `world` contiguous line
    ranges (sharding.strong_block_for_rank = split_at_newlines semantics), database replicated, no data-path collective.
    Reported separately: `value` = the whole job from HBM-resident input (every rank's range uploaded before the timed
    region, scanned in batches of <= --batch-lines lines), and `end_to_end` = the same ranges' first batches from pinned host
    memory through two scanners on two streams per GPU (H2D of one batch under the kernels of the other)."""
    import threading
    import matchy_amd as M
    from matchy_amd import sharding
    from tools import synth
    cfg = synth.config(args.config)
    blob = synth.build_db(cfg)
    db = M.Database(blob)
    blk = sharding.strong_block_for_rank(rank, world, args.lines)
    per = args.batch_lines
    batches = [(blk.first_line + o, min(per, blk.n_lines - o)) for o in range(0, blk.n_lines, per)]
    # generate (all host cores of this rank's share, the generator is counter-based) and upload, batch by batch
    cap = per * 200 + (1 << 20)
    dlog = torch.empty(len(batches) * cap, dtype=torch.uint8, device=dev)
    stage = torch.empty(cap, dtype=torch.uint8).pin_memory()
    keep_host = []                       # the first batches stay in pinned host memory for the end-to-end measurement
    sizes, lines_total = [], 0
    nthreads = max(1, min(16, len(os.sched_getaffinity(0)) // max(1, min(world, 8))))
    for bi, (first, n) in enumerate(batches):
        # sub-blocks generated in parallel straight into the pinned stage; they are contiguous because every sub-block is
        # sized first (the generator reports the bytes it needs)
        sub = [(first + k * (n // nthreads), (n // nthreads) if k < nthreads - 1 else n - (nthreads - 1) * (n // nthreads)) for k in range(nthreads)]
        need = [0] * nthreads
        def size_of(k):
            need[k] = synth.make_log_into(cfg, sub[k][0], sub[k][1], 0, 0) if sub[k][1] else 0
        ths = [threading.Thread(target=size_of, args=(k,)) for k in range(nthreads)]
        [t.start() for t in ths]; [t.join() for t in ths]
        offs = [sum(need[:k]) for k in range(nthreads)]
        total = sum(need)
        if total > cap:
            raise SystemExit("batch larger than its buffer: lower --batch-lines")
        def gen(k):
            if sub[k][1]:
                synth.make_log_into(cfg, sub[k][0], sub[k][1], stage.data_ptr() + offs[k], need[k])
        ths = [threading.Thread(target=gen, args=(k,)) for k in range(nthreads)]
        [t.start() for t in ths]; [t.join() for t in ths]
        dlog[bi * cap: bi * cap + total].copy_(stage[:total])
        torch.cuda.synchronize()
        if args.full and len(keep_host) < args.e2e_batches:
            h = torch.empty(total, dtype=torch.uint8).pin_memory()
            h.copy_(stage[:total])
            keep_host.append(h)
        sizes.append(total)
        lines_total += n
    nbytes = sum(sizes)
    stream = torch.cuda.current_stream().cuda_stream
    scanner = M.Scanner(db, device=local_rank, profile=True)

    def one_pass():
        ln = cand = hits = 0
        kms = 0.0
        for bi, sz in enumerate(sizes):
            r = scanner.scan_device(dlog.data_ptr() + bi * cap, sz, stream=stream, fetch_mode=fetch_hits)
            ln += r.lines; cand += r.candidates; hits += r.n_hits
            r.close()
            kms += scanner.timing_ms()["total"]
        return ln, cand, hits, kms

    def barrier():
        sharding.barrier(dist, world, torch.cuda.synchronize)
    for _ in range(max(1, args.warmup)):
        counts = one_pass()
    barrier()
    t0 = time.perf_counter()
    kernel_ms = 0.0
    for _ in range(args.steps):
        counts = one_pass()
        kernel_ms += counts[3]
    barrier()
    elapsed = time.perf_counter() - t0
    agg = sharding.aggregate(dist, world, coll_dev, elapsed, nbytes, counts[0], counts[2], counts[1])
    kagg = sharding.aggregate(dist, world, coll_dev, kernel_ms * 1e-3, 0, 0, 0, 0)
    # ---- --dump-outputs: rank 0's records of a pass are only readable batch by batch, so the pass runs once more, untimed, and
    # every batch's records are kept (same input, same records in canonical order); hits.npy carries the batch as a first column
    if args.dump_outputs is not None and rank == 0:
        import numpy as np
        all_hits, all_ids, n_rows = [], [], 0
        for bi, sz in enumerate(sizes):
            r = scanner.scan_device(dlog.data_ptr() + bi * cap, sz, stream=stream, fetch_mode=fetch_hits)
            h, ids = hit_arrays(r)
            r.close()
            all_hits.append(np.hstack([np.full((len(h), 1), bi, dtype=np.float64), h]))
            ids[:, 0] += n_rows
            all_ids.append(ids)
            n_rows += len(h)
        dump_outputs(args.dump_outputs, counts[:3], np.vstack(all_hits), np.vstack(all_ids))
    # ---- end to end from pinned host memory: two scanners, two threads, alternating batches
    e2e = None
    if keep_host:
        scs = [M.Scanner(db, device=local_rank), M.Scanner(db, device=local_rank)]
        def worker(w, out):
            n = 0
            for bi in range(w, len(keep_host), 2):
                r = scs[w].scan_ptr(keep_host[bi].data_ptr(), keep_host[bi].numel())
                n += r.n_hits
                r.close()
            out[w] = n
        for rep in range(2):   # first repetition warms the staging buffers
            out = [0, 0]
            barrier()
            te = time.perf_counter()
            ths = [threading.Thread(target=worker, args=(w, out)) for w in range(2)]
            [t.start() for t in ths]; [t.join() for t in ths]
            barrier()
            te = time.perf_counter() - te
        eb = sum(h.numel() for h in keep_host)
        eagg = sharding.aggregate(dist, world, coll_dev, te, eb, 0, sum(out), 0)
        e2e = {"value": round(eagg["bytes"] / eagg["elapsed_s"] / 1e9, 2), "unit": "GB/s", "bytes": eagg["bytes"],
               "entry": "matchy_scanner_scan from pinned host memory, two scanners per GPU on their own streams, H2D included"}
        for sc in scs:
            sc.close()
    # same-run parity on the head of the job: the first lines of rank 0's first batch (the generator is a pure function of the line
    # index, so the sample is generated again on the host) through the same scanner and through the oracle
    parity = None
    if args.full and rank == 0 and not args.no_cpu:
        from oracle import oracle
        n_par = min(args.cpu_lines, batches[0][1], 1_000_000)
        sample = synth.make_log(cfg, batches[0][0], n_par)
        ohits, _, ost = oracle.Database(blob).scan(sample, threads=min(len(os.sched_getaffinity(0)), 16), cache=0, want_json=False)
        r = scanner.scan(sample)
        parity = "ok" if (r.hits() == ohits and (r.lines, r.candidates) == (ost.lines, ost.candidates)) else f"MISMATCH gpu={r.n_hits} cpu={len(ohits)}"
        r.close()
    if rank == 0:
        step_s = agg["elapsed_s"] / args.steps
        print(json.dumps({
            "metric": "log GB/s scanned (matchy match hot path, 100K IoCs)", "value": round(agg["bytes"] / step_s / 1e9, 3), "unit": "GB/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_s * 1e3, 3), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "u8", "data": "synthetic", "parity_vs_oracle": parity,
            "batches": len(batches), "per_batch_ms": round(step_s * 1e3 / max(1, len(batches)), 4),
            "config": {"workload": f"BASELINE configs[3]-style strong scaling: ONE job of {args.lines} nginx-style lines ({agg['bytes']} B), config {args.config}, "
                                   f"cut into {world} contiguous newline-aligned ranges, batches of <= {per} lines, DB replicated, no collective",
                       "total_lines": args.lines, "total_bytes": agg["bytes"]},
            "lines_per_s": round(agg["lines"] / step_s, 1), "hits_per_step": agg["hits"], "candidates_per_step": agg["candidates"],
            "kernel_only": {"value": round(agg["bytes"] / (kagg["elapsed_s"] / args.steps) / 1e9, 3), "unit": "GB/s",
                            "note": "sum of the kernel time of all batches on the slowest rank (HIP events), input resident in HBM"},
            "end_to_end": e2e}))
    scanner.close()


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nproc-per-node N bench.py <same
    arguments>` as a child (rendezvous on 127.0.0.1, a free port) and return its exit status. Rank 0's JSON line reaches stdout
    through the inherited descriptors. Reference: the worker fan-out of crates/matchy/src/processing/parallel.rs:594-704."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), *sys.argv[1:]]
    return subprocess.run(cmd).returncode


def dry_run(args, rank, world):
    """BENCH_DRYRUN=1: the launch plumbing without a GPU (CPU test of `--gpus N`): rendezvous over gloo, the barrier and the
    reduction bench.py uses, one JSON line from rank 0 with `value` null. Measures nothing."""
    import torch
    import torch.distributed as dist
    from matchy_amd import sharding
    if world > 1:
        dist.init_process_group(backend="gloo")
    sharding.barrier(dist, world)
    blk = sharding.block_for_rank(rank, world, args.lines)
    agg = sharding.aggregate(dist, world, torch.device("cpu"), 1.0, 0, blk.n_lines, 0, 0)
    if rank == 0:
        print(json.dumps({"metric": "log GB/s scanned (matchy match hot path, 100K IoCs)", "value": None, "unit": "GB/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "dry_run": True, "lines": agg["lines"]}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)   # a step is ~1.2 ms: 50 of them keep one slow step (host jitter) out of the average
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lines", type=int, default=10_000_000, help="log lines per GPU (BASELINE config: 10M)")
    ap.add_argument("--config", default="c2", help="indicator mix (tools/synth.py): c2 = 100K mixed IoCs")
    ap.add_argument("--cpu-lines", type=int, default=3_000_000, help="lines of the same log timed on the CPU oracle (rank 0, N=1)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the PCIe-inclusive host-buffer measurement")
    ap.add_argument("--case-insensitive", action="store_true", help="build the database with match_mode 1 (matchy build -i)")
    ap.add_argument("--pipelined", type=int, default=3, help="--full, N > 1: after the timed steps, time the same K steps again with N batches in flight per GPU "
                    "(scanners on their own streams) and report it as the extra object `pipelined` (never as `value`). 0 / 1 = skip "
                    "(tools/prof.sh does, so that a profile shows every kernel of a step running alone)")
    ap.add_argument("--records", choices=["compact", "full"], default="compact", help="host-resident hit records of the timed steps: compact = IPv4 results "
                    "as 8-byte records (MATCHY_SCAN_FETCH_HITS | MATCHY_SCAN_FETCH_COMPACT), everything else 16 bytes; full = 16 bytes for every hit")
    ap.add_argument("--slices", type=int, default=0, help="matchy_scanner_set_slices: 0 = the library's default for the batch size, 1 = one launch of every "
                    "kernel over the whole batch, n = n equal slices")
    ap.add_argument("--extract-flags", type=int, default=0, help="diagnostics only: MATCHY_EXTRACT_* bit mask (0 = what the DB needs)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak", help="strong: --lines is the size of ONE job that is cut across the GPUs "
                    "(default 100 M lines of --config c4 = BASELINE configs[3])")
    ap.add_argument("--batch-lines", type=int, default=10_000_000, help="strong scaling: lines per batch (a batch must stay below 2 GiB; the default is the weak line's batch)")
    ap.add_argument("--e2e-batches", type=int, default=4, help="strong scaling: batches per rank kept in pinned host memory for the end-to-end measurement")
    ap.add_argument("--log-shape", default="nginx", choices=["nginx", "jsonl-app", "ip-dense", "url-heavy", "hash-dense", "skewed-halves"],
                    help="shape of the synthetic log (tools/synthgen.cpp): nginx = the BASELINE workload; the others answer 'what does the number do on other "
                         "input' (BASELINE.md §3). skewed-halves: the first half of every rank's block is prose with nothing to extract, the second half is ip-dense")
    ap.add_argument("--no-scatter-gather", action="store_true", help="skip the one-process scatter / gather leg (matchy_multi_scanner over all GPUs of the job)")
    ap.add_argument("--full", action="store_true", help="after the headline steps, run every other leg as well: records left in HBM, batches in flight "
                    "(--pipelined), the measured copy peak, the host-buffer entry, scatter / gather, the CPU baselines and the same-run parity check "
                    "(strong scaling: end to end and parity). Without it a run sets up, warms up, times --steps steps and prints the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step returned to its caller as DIR/<name>.npy "
                    "(float64): counts.npy = [lines, candidates, hits]; hits.npy = one row per hit record [start, end, item type, kind (0 ip, 1 pattern), "
                    "prefix_len, ip_data_offset] in canonical order; hit_ids.npy = [row of hits.npy, pattern id, data offset] per pattern id. Above "
                    f"{DUMP_LIMIT >> 20} MB in all, a fixed seeded sample of the hit rows is written. --scaling strong: every batch of a pass, "
                    "with the batch index as the first column of hits.npy")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if args.scaling == "strong":
        if "--lines" not in " ".join(sys.argv):
            args.lines = 100_000_000
        if "--config" not in " ".join(sys.argv):
            args.config = "c4"
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    global fetch_hits
    fetch_hits = 9 if args.records == "compact" else 1   # MATCHY_SCAN_FETCH_HITS [| MATCHY_SCAN_FETCH_COMPACT]

    # --gpus N is what runs. Started by torch.distributed.run (WORLD_SIZE set): the launcher's world must be N. Started
    # directly with N > 1: this process becomes the launcher — one rank per GPU as a CHILD process tree, started before
    # anything here has imported torch or touched HIP — and relays the ranks' output and exit status.
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            sys.exit(spawn_ranks(args.gpus))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # BENCH_REHEARSE=1: rehearsal of the multi-rank path on a box with ONE GPU — every rank uses device 0 and the two
    # collectives (barrier, reduction of the per-rank scalars) run over gloo on the CPU. The numbers of such a run mean nothing.
    rehearse = os.environ.get("BENCH_REHEARSE") == "1"
    if rehearse:
        local_rank = 0
    os.environ["MATCHY_AMD_DEVICE"] = str(local_rank)

    if os.environ.get("BENCH_DRYRUN") == "1":
        return dry_run(args, rank, world)

    import torch
    import torch.distributed as dist

    if not rehearse and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: --gpus {world} but only {torch.cuda.device_count()} device(s) are visible")
    if world > 1:
        if rehearse:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    coll_dev = torch.device("cpu") if rehearse else dev   # where the reduced scalars live
    if args.scaling == "strong":
        run_strong(args, rank, local_rank, world, rehearse, torch, dist, dev, coll_dev)
        if world > 1:
            dist.destroy_process_group()
        return

    import matchy_amd as M
    from matchy_amd import sharding
    from tools import synth

    # This rank feeds its GPU from host memory (the upload of the batch, the end-to-end legs): it runs on the CPUs of the GPU's NUMA node —
    # sched_setaffinity in this process (matchy_amd_bind_thread_to_device), never an exec — so that the pages it touches and pins are local
    # to the socket the GPU hangs off (two-socket 8-GPU nodes: SURVEY §8e caveat).
    numa = None
    if not rehearse:
        ML = M.lib()
        cpus_before = len(os.sched_getaffinity(0))
        numa = {"node": int(ML.matchy_amd_device_numa_node(local_rank)), "cpus_bound": int(ML.matchy_amd_bind_thread_to_device(local_rank)),
                "cpus_before": cpus_before}

    cfg = synth.config(args.config)
    base_name = args.config.split("/")[0]
    cfg_index = {"c1": 0, "c2": 1, "c3": 2, "c3b": 2, "c4": 3, "c5": 4}[base_name]
    cfg_note = (" (AC-forced variant, glob: keys)" if base_name == "c3b" else "") + (f" (indicators scaled 1/{args.config.split('/')[1]})" if "/" in args.config else "")
    blob = synth.build_db(cfg, case_insensitive=args.case_insensitive)
    if args.case_insensitive:
        cfg_note += " (case-insensitive database)"
    db = M.Database(blob)
    scanner = M.Scanner(db, extract_flags=args.extract_flags, device=local_rank, profile=True)
    if args.slices:
        scanner.set_slices(args.slices)

    # ---- synthetic batch: this rank's line block, generated on the host, uploaded once
    shape = args.log_shape
    if shape != "nginx":
        # other shapes have other line lengths: as many lines as keep the batch near the nginx batch's size and below the 2 GiB launch limit
        probe = len(synth.make_log(cfg, 0, 5000, shape, 10000)) + len(synth.make_log(cfg, 5000, 5000, shape, 10000))
        args.lines = min(args.lines, int(1.85e9 / (probe / 10000.0)))
    shape_param = args.lines if shape == "skewed-halves" else 0   # period = the rank's block: first half sparse, second half dense
    first_line = sharding.block_for_rank(rank, world, args.lines).first_line
    cap = args.lines * 200 + (1 << 20)
    host = torch.empty(cap, dtype=torch.uint8)
    nbytes = synth.make_log_into(cfg, first_line, args.lines, host.data_ptr(), cap, shape, shape_param)
    if nbytes > cap:
        host = torch.empty(nbytes, dtype=torch.uint8)
        nbytes = synth.make_log_into(cfg, first_line, args.lines, host.data_ptr(), nbytes, shape, shape_param)
    if nbytes >= 0x7FFF0000:
        raise SystemExit("batch exceeds the 2 GiB single-launch limit; lower --lines")
    dlog = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    dlog[:nbytes].copy_(host[:nbytes])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    last_res = [None]

    def step(keep=False):
        res = scanner.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=fetch_hits)
        out = (res.lines, res.candidates, res.n_hits)
        if keep:
            last_res[0] = res   # --dump-outputs: the records stay readable until the scanner's next scan
        else:
            res.close()
        return out

    # --pipelined N > 1: N scanners, each on its own stream; a step submits a batch to the next scanner after collecting
    # that scanner's previous batch, so up to N batches overlap (one batch's latency-bound kernels and result transfer
    # under another's streaming kernel). Every batch is complete — results in host memory — when its wait returns.
    # The extra scanners (and their streams) are created when that leg starts, behind the headline measurement: the runtime maps
    # streams onto a few hardware queues in creation order, and more streams than queues make the side streams of the forked
    # headline scan share queues (measured: tail 0.237 -> 0.281 ms with two idle scanners around).
    scanners = [scanner]
    streams = [stream]
    tstreams = []

    def make_pipeline_scanners():
        for _ in range(1, max(1, args.pipelined)):
            scanners.append(M.Scanner(db, extract_flags=args.extract_flags, device=local_rank, profile=True))
            ts = torch.cuda.Stream(device=dev)
            tstreams.append(ts)
            streams.append(ts.cuda_stream)
        busy.extend([False] * (len(scanners) - len(busy)))
    busy = [False] * len(scanners)
    turn = [0]
    last = [None]

    def collect(i):
        res = scanners[i].wait()
        last[0] = (res.lines, res.candidates, res.n_hits)
        res.close()
        busy[i] = False

    def step_pipelined():
        i = turn[0] % len(scanners)
        turn[0] += 1
        if busy[i]:
            collect(i)
        scanners[i].submit_device(dlog.data_ptr(), nbytes, stream=streams[i], fetch_mode=fetch_hits)
        busy[i] = True

    def drain():
        for i in range(len(scanners)):
            if busy[i]:
                collect(i)
        return last[0]

    def barrier():
        sharding.barrier(dist, world, torch.cuda.synchronize)

    # one-time runtime initialisation (pinned result buffer, the runtime's D2H engine set-up shows up as one slow copy
    # within the first few scans) is part of set-up, like the upload of the batch; then the W warm-up steps
    for _ in range(10):
        counts = step()
    for _ in range(args.warmup):
        counts = step()
    tok_ms, look_ms, rare_ms, val_ms = [], [], [], []
    dump_last = args.dump_outputs is not None and rank == 0
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ts0 = time.perf_counter()
        counts = step(keep=dump_last and i == args.steps - 1)
        if os.environ.get("BENCH_DEBUG"):
            print(f"step {1e3 * (time.perf_counter() - ts0):.3f} ms", file=sys.stderr)
        t = scanner.timing_ms()
        tok_ms.append(t["anchor"]); look_ms.append(t["lookup"]); rare_ms.append(t["rare"]); val_ms.append(t["validate"])
    scanner.last_slices_timed = scanner.last_slices()
    barrier()
    elapsed = time.perf_counter() - t0
    agg = sharding.aggregate(dist, world, coll_dev, elapsed, nbytes, counts[0], counts[2], counts[1])
    elapsed = agg["elapsed_s"]
    total_bytes, total_lines = float(agg["bytes"]), float(agg["lines"])

    ms_per_step = elapsed / args.steps * 1e3
    value = total_bytes / (elapsed / args.steps) / 1e9

    # ---- --dump-outputs: what the last timed step handed its caller (rank 0's batch)
    if last_res[0] is not None:
        dump_outputs(args.dump_outputs, counts, *hit_arrays(last_res[0]))
        last_res[0].close()

    # ---- the same K steps with the hit records left in device memory (MATCHY_SCAN_FETCH_DEVICE): what a consumer that stays on
    # the GPU gets, and the only way a workload where nearly every line hits is not bound by 16 bytes per hit over PCIe
    def step_dev():
        res = scanner.scan_device(dlog.data_ptr(), nbytes, stream=stream, fetch_mode=4)
        out = (res.lines, res.candidates, res.n_hits)
        res.close()
        return out
    device_results = None
    if args.full:
        for _ in range(2):
            dcounts = step_dev()
        barrier()
        td0 = time.perf_counter()
        for _ in range(args.steps):
            dcounts = step_dev()
        barrier()
        tdev = time.perf_counter() - td0
        dagg = sharding.aggregate(dist, world, coll_dev, tdev, nbytes, dcounts[0], dcounts[2], dcounts[1])
        device_results = {"value": round(float(dagg["bytes"]) / (dagg["elapsed_s"] / args.steps) / 1e9, 3), "unit": "GB/s",
                          "ms_per_step": round(dagg["elapsed_s"] / args.steps * 1e3, 4), "same_counts": bool(tuple(dcounts) == tuple(counts)),
                          "note": "hit records stay in HBM (fetch_mode 4); `value` above moves them to host memory"}

    # ---- the same K steps once more with several batches in flight (how a streaming host drives the scanners: submit /
    # wait, one stream per scanner). Reported beside the headline numbers, never instead of them: with overlapping
    # batches the kernels time-share the GPU and their individual durations say nothing about the kernels.
    pipelined = None
    if args.full and args.pipelined > 1:
        make_pipeline_scanners()
        for _ in range(2 * len(scanners)):
            step_pipelined()
        drain()
        barrier()
        tp0 = time.perf_counter()
        for _ in range(args.steps):
            step_pipelined()
        pcounts = drain()
        barrier()
        pel = time.perf_counter() - tp0
        pagg = sharding.aggregate(dist, world, coll_dev, pel, nbytes, pcounts[0], pcounts[2], pcounts[1])
        pipelined = {"batches_in_flight": len(scanners), "value": round(float(pagg["bytes"]) / (pagg["elapsed_s"] / args.steps) / 1e9, 3), "unit": "GB/s",
                     "ms_per_step": round(pagg["elapsed_s"] / args.steps * 1e3, 4), "steps": args.steps,
                     "same_counts": bool(tuple(pcounts) == tuple(counts))}
    # Roofline: the unit of work is the log byte, read once: algorithmic bytes per launch = len(log) for
    # every kernel of the pass (each launch covers the whole batch). `roofline` is the DOMINANT (slowest) kernel,
    # timed live with HIP events on the launch stream; `roofline_pipeline` prices the sum of all kernels of one pass.
    if sum(rare_ms) == 0 and sum(look_ms) == 0:
        # forked scan (matchy_scanner_scan_device): the kernels behind k_anchor run on three streams and are timed as ONE interval
        kern = {"k_anchor": sum(tok_ms) / len(tok_ms), "tail (k_validate_dom, k_validate, k_lookup; k_lookup_ip, k_rare beside)": sum(val_ms) / len(val_ms)}
    else:
        kern = {"k_anchor": sum(tok_ms) / len(tok_ms), "k_validate_dom+k_validate": sum(val_ms) / len(val_ms),
                "k_rare": sum(rare_ms) / len(rare_ms), "k_lookup": sum(look_ms) / len(look_ms)}
    # `roofline` prices ONE kernel: k_anchor, the streaming pass (the only kernel that reads the log, and the longest single kernel
    # of every configuration). In a forked scan the other entry of `kern` is an interval over several kernels on several streams:
    # never a roofline candidate. In a single-stream scan a longer single kernel would take its place.
    singles = {k: v for k, v in kern.items() if not k.startswith("tail")}
    dom_name = max(singles, key=singles.get)
    achieved = nbytes / (kern[dom_name] * 1e-3) / 1e9
    pipe_ms = sum(kern.values())
    pipe_achieved = nbytes / (pipe_ms * 1e-3) / 1e9
    traffic = None
    tr_note = None
    try:
        # HBM bytes per launch from the newest committed rocprofv3 --pmc passes of this command (tools/prof.sh: separate
        # FETCH_SIZE / WRITE_SIZE runs, FETCH_SIZE x2 on gfx950). The file carries a fingerprint of the kernel sources it was
        # taken from; a file from other sources, or of another batch size, is refused (traffic = null) instead of quoted.
        from tools.csrc_hash import csrc_sha
        files = sorted((ROOT / "profiles").glob("r*_traffic.json"))
        tj = json.load(open(files[-1])) if files else {}
        if tj.get("bytes_per_gpu") == nbytes and tj.get("csrc_sha") == csrc_sha():
            prefix = {"k_anchor": "mxy::k_anchor", "k_validate_dom+k_validate": "mxy::k_validate_dom", "k_rare": "mxy::k_rare", "k_lookup": "mxy::k_lookup"}[dom_name]
            keys = [k for k in tj["kernels"] if k.startswith(prefix)]
            if len(keys) == 1:   # exactly one instantiation of the dominant kernel ran in the profiled command
                traffic = tj["kernels"][keys[0]]["hbm_bytes"]
                tr_note = f"profiles/{files[-1].name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same command, kernel sources {tj['csrc_sha']} (= this tree)"
        elif files:
            tr_note = f"profiles/{files[-1].name} refused: taken from other kernel sources or another batch size"
    except (OSError, ValueError, KeyError, ImportError) as ex:
        tr_note = f"traffic file not usable: {type(ex).__name__}: {ex}"

    # ---- the box's own copy bandwidth, measured in this run (report the spec peak and the measured one)
    peak_measured = None
    if args.full and rank == 0:
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
        peak_measured = round(5 * 2 * nb / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
        del a, b

    # ---- PCIe-inclusive rate of the host-buffer entry (matchy_scanner_scan from pinned host memory: H2D in < 1 GiB pieces,
    # scan, canonical-order sort on the GPU, hit records back). Reported beside the headline, never as `value`.
    end_to_end = None
    if args.full and rank == 0 and world == 1 and not args.no_e2e:
        pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        pinned.copy_(host[:nbytes])
        sc2 = M.Scanner(db, extract_flags=args.extract_flags, device=local_rank)
        times = []
        for rep in range(4):
            te = time.perf_counter()
            r = sc2.scan_ptr(pinned.data_ptr(), nbytes)
            times.append(time.perf_counter() - te)
            e2e_counts = (r.lines, r.n_hits)
            r.close()
        sc2.close()
        best = min(times[1:])
        end_to_end = {"value": round(nbytes / best / 1e9, 2), "unit": "GB/s", "ms": round(best * 1e3, 2), "entry": "matchy_scanner_scan, pinned host buffer, H2D included",
                      "same_counts": bool(e2e_counts == (counts[0], counts[2]))}
        del pinned

    # ---- one-process scatter / gather over every GPU of the job (north_star: line blocks sharded across the GPUs of one node by the
    # host, no collective): rank 0 drives matchy_multi_scanner_* — one worker thread per device entry, each bound to its GPU's NUMA
    # node — with ONE job of `world` blocks in pinned host memory, cut into newline-aligned 256 MiB batches that are handed out in
    # sequence and gathered in sequence, results (canonical-order records) in host memory. value = job bytes / wall time of the
    # best of three passes. The other ranks wait at the barrier (their GPUs are driven by rank 0's workers meanwhile). Every block
    # is this rank's 10 M lines again: generating `world` different blocks would take longer than the driver's run, and the
    # mechanics — H2D per device, scan, ordered gather — do not depend on the bytes.
    scatter_gather = None
    if args.full and not args.no_scatter_gather:
        barrier()
        if rank == 0:
            import numpy as np
            import threading
            hv = host[:nbytes].numpy()
            cuts = [0]
            step_b = 256 << 20
            while cuts[-1] + step_b < nbytes:
                want = cuts[-1] + step_b
                back = np.flatnonzero(hv[want - (1 << 16):want] == 10)
                cuts.append(want - (1 << 16) + int(back[-1]) + 1 if len(back) else want)
            cuts.append(nbytes)
            pieces = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1) if cuts[i + 1] > cuts[i]]
            gpus = [0] * world if rehearse else list(range(world))
            devs = gpus * 2   # two scanners per GPU: one copies while the other post-processes
            # ONE pinned copy of the block PER NUMA NODE that has GPUs of this job, allocated and filled (first touch) by a thread
            # bound to that node's CPUs: a GPU then pulls its batches from the memory of its own socket. (Round 4 fed every GPU from
            # one buffer on rank 0's node: on a two-socket node half the copies crossed the socket link.) The main thread, which only
            # submits and gathers, goes back to the process's whole affinity for this leg.
            ML = M.lib()
            node_of_gpu = [int(ML.matchy_amd_device_numa_node(g)) for g in gpus]
            buffers = {}   # node -> pinned tensor

            def alloc_on(node, gpu):
                bound = int(ML.matchy_amd_bind_thread_to_device(gpu)) if not rehearse else 0
                t = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
                t.copy_(host[:nbytes])
                buffers[node] = (t, bound)

            for node in sorted(set(node_of_gpu)):
                th = threading.Thread(target=alloc_on, args=(node, gpus[node_of_gpu.index(node)]))
                th.start(); th.join()
            if not rehearse:
                ML.matchy_amd_unbind_thread()
            ms = M.MultiScanner(db, devices=devs, extract_flags=args.extract_flags)
            limit = ms.max_pending()
            times, sg_counts = [], None
            for rep in range(4):
                tsg = time.perf_counter()
                tl = tc = th_ = 0

                def take():
                    nonlocal tl, tc, th_
                    b = ms.next()
                    tl += b["lines"]; tc += b["candidates"]; th_ += b["n_hits"]

                for blk in range(world):
                    node = node_of_gpu[blk]          # block `blk` is GPU blk's share of the job: it lives on that GPU's node
                    base = buffers[node][0].data_ptr()
                    for off, n in pieces:
                        # one thread submits and gathers: take a batch back whenever the in-flight bound is reached (back-pressure:
                        # at most 2 x workers + 2 batches exist between submit and next)
                        while ms.pending() >= limit:
                            take()
                        ms.submit_ptr(base + off, n, tag=blk, numa_node=node)
                while ms.pending():
                    take()
                times.append(time.perf_counter() - tsg)
                sg_counts = (tl, tc, th_)
            worker_numa = ms.worker_numa()
            ms.close()
            best = min(times[1:])
            scatter_gather = {"value": round(world * nbytes / best / 1e9, 2), "unit": "GB/s", "ms": round(best * 1e3, 2), "job_bytes": world * nbytes,
                              "devices": devs, "batches": len(pieces) * world, "max_pending": limit,
                              "numa": {"buffers": [{"node": n_, "bytes": nbytes, "allocating_thread_cpus": b_[1]} for n_, b_ in sorted(buffers.items())],
                                       "gpu_nodes": node_of_gpu,
                                       "workers": [{"device": devs[w], "node": wn[0], "cpus_bound": wn[1]} for w, wn in enumerate(worker_numa)]},
                              "entry": "matchy_multi_scanner_submit_near / _next: one process, one pinned copy of the block per NUMA node -> per-device H2D from the local node -> scan -> records gathered in submission order",
                              "same_counts": bool(sg_counts == (world * counts[0], world * counts[1], world * counts[2]))}
            buffers.clear()
            if not rehearse:
                ML.matchy_amd_bind_thread_to_device(local_rank)
        barrier()

    cpu = None
    cpu_t1 = None
    cpu_all = None
    parity = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu:
        # ---- CPU baseline: the oracle ("port" of the reference CPU path) on a bounded sample of the SAME log,
        # all host cores, newline-aligned chunks + 10 000-entry per-thread LRU like `matchy match` defaults.
        from oracle import oracle
        n_cpu_lines = min(args.cpu_lines, args.lines)
        # sample = first n_cpu_lines lines of this rank's batch
        hv = host[:nbytes].numpy()
        import numpy as np
        nl = np.flatnonzero(hv[: min(nbytes, n_cpu_lines * 400)] == 10)
        sample_end = int(nl[n_cpu_lines - 1]) + 1 if len(nl) >= n_cpu_lines else nbytes
        sample = hv[:sample_end].tobytes()
        odb = oracle.Database(blob)
        cores = min(len(os.sched_getaffinity(0)), 16)  # GPU box share: 16 host cores per GPU
        ohits, _, st = odb.scan(sample, threads=cores, cache=10000, want_json=False)
        cpu = {"value": round(len(sample) / st.seconds / 1e9, 4), "unit": "GB/s", "cores": cores, "kind": "port", "host_cpus": os.cpu_count(),
               "affinity_cpus": len(os.sched_getaffinity(0)),
               "sample": f"first {n_cpu_lines} lines ({len(sample)} B) of the same log, {cores} threads, 256 KiB newline-aligned chunks, LRU 10000",
               "lines_per_s": round(st.lines / st.seconds, 1)}
        # ... and at T = every CPU this process may run on (SURVEY §8d "T = all host cores"; reference: available_parallelism workers,
        # crates/matchy/src/bin/match_processor/parallel.rs:134-138 and the chunk sizes of processing/parallel.rs:107-123). On the GPU
        # boxes the affinity mask is the whole machine while the pod's CPU share is smaller: the figure is what the box gives THIS
        # process with that many threads, `cores` says how many were started.
        all_cores = len(os.sched_getaffinity(0))
        if all_cores != cores:
            _, _, sta = odb.scan(sample, threads=all_cores, cache=10000, want_json=False)
            cpu_all = {"value": round(len(sample) / sta.seconds / 1e9, 4), "unit": "GB/s", "cores": all_cores, "kind": "port",
                       "sample": f"the same {n_cpu_lines} lines, {all_cores} threads (= affinity_cpus), 256 KiB newline-aligned chunks, LRU 10000",
                       "lines_per_s": round(sta.lines / sta.seconds, 1)}
        else:
            cpu_all = dict(cpu, sample=cpu["sample"] + " (= affinity_cpus: the same run)")
        # the same path on ONE core (T = all cores and T = 1), on a tenth of the sample
        n1 = max(1, n_cpu_lines // 10)
        s1_end = int(nl[n1 - 1]) + 1 if len(nl) >= n1 else sample_end
        _, _, st1 = odb.scan(sample[:s1_end], threads=1, cache=10000, want_json=False)
        cpu_t1 = {"value": round(s1_end / st1.seconds / 1e9, 4), "unit": "GB/s", "cores": 1, "kind": "port",
                  "sample": f"first {n1} lines ({s1_end} B) of the same log, 1 thread, LRU 10000", "lines_per_s": round(st1.lines / st1.seconds, 1)}
        # parity in the same run: GPU hits on the sample == oracle hits
        res = scanner.scan_device(dlog.data_ptr(), sample_end, stream=stream, fetch_mode=3)
        ghits = res.hits()
        res.close()
        parity = "ok" if ghits == ohits else f"MISMATCH gpu={len(ghits)} cpu={len(ohits)}"
        # ... and the records as the timed steps fetch them (device order; compact IPv4 records expanded): the same set
        res = scanner.scan_device(dlog.data_ptr(), sample_end, stream=stream, fetch_mode=fetch_hits)
        key = lambda h: (h["start"], h["end"], h["type"], h["kind"], h["prefix_len"], h["ip_data_offset"])
        if sorted(res.hits(), key=key) != sorted(ohits, key=key):
            parity = f"MISMATCH in the timed fetch mode ({args.records} records)"
        res.close()

    if rank == 0:
        out = {
            "metric": "log GB/s scanned (matchy match hot path, 100K IoCs)",
            "value": round(value, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {"workload": f"BASELINE configs[{cfg_index}]{cfg_note}: {cfg.n_ip + cfg.n_cidr + cfg.n_dom + cfg.n_hash + cfg.n_glob} mixed IoCs "
                                   f"({cfg.n_ip} IPv4 + {cfg.n_cidr} CIDR + {cfg.n_dom} domains + {cfg.n_hash} hashes + {cfg.n_glob} globs), "
                                   f"{args.lines} {'nginx-style' if shape == 'nginx' else shape + '-shaped'} lines per GPU",
                       "log_shape": shape,
                       "lines_per_gpu": args.lines, "bytes_per_gpu": nbytes, "sharding": "line-block per GPU, DB replicated, no collective"},
            "lines_per_s": round(total_lines / (elapsed / args.steps), 1),
            "candidates_per_step": agg["candidates"],
            "hits_per_step": agg["hits"],
            "slices": scanner.last_slices_timed,
            "records": args.records + (" (IPv4 results as 8-byte records: matchy_scan_ip4_hit_t; in host memory when a step ends)" if args.records == "compact"
                                       else " (16-byte matchy_scan_hit_t for every hit; in host memory when a step ends)"),
            "kernel_ms": {k: round(v, 4) for k, v in kern.items()},
            "kernel_ms_note": "HIP-event intervals on the scan's stream: k_anchor alone (it also looks the sparse IPv4 candidates up), then everything "
                              "behind it as one interval (k_validate_dom -> k_lookup on the scan's stream; tokens / IPv6 / e-mail, the undecided domains "
                              "and k_rare with their own lookups on three side streams); per-kernel durations: profiles/r04_bench_c2_summary.txt, r04_step_timeline.txt",
            "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "peak_measured": peak_measured, "peak_measured_note": "device-to-device copy of 1 GiB in this run (--full), read + write bytes / time",
                         "traffic": traffic, "kernel": dom_name, "algorithmic_bytes_per_launch": nbytes, "traffic_source": tr_note},
            "roofline_pipeline": {"bound": "hbm", "achieved": round(pipe_achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(pipe_achieved / HBM_PEAK_GBS, 4), "kernels_ms": round(pipe_ms, 4)},
            "numa": numa,
        }
        if args.full:
            # the legs only a --full run measures
            out.update({
                "cpu_baseline": cpu,
                "cpu_baseline_t1": cpu_t1,
                "cpu_baseline_all": cpu_all,
                # what the reference documents for itself (unstated hardware) — the oracle port above is a restatement, not the
                # Rust binary, and its single-thread rate is below these ranges: read the GPU/CPU ratio against BOTH
                "reference_documented": {"extractor_single_thread_MBps": "~450 (DEVELOPMENT.md:266)", "match_sequential_MBps": "200-500 (book/src/commands/matchy-match.md:343)",
                                         "match_parallel_MBps": "400-2000 depending on core count (matchy-match.md:344)",
                                         "extract_plus_lookup_MBps": "100-300 (book/src/guide/querying.md:187)"} if cpu else None,
                "end_to_end": end_to_end,
                "scatter_gather": scatter_gather,
                "device_results": device_results,
                "pipelined": pipelined,
                "parity_vs_oracle": parity,
            })
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
