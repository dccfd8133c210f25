"""What the unescape front pass (csrc/unescape.hip) costs.

Three inputs of --mib MiB each, resident in device memory, through matchy_scanner_scan_escaped, counters only; the three steps are timed
by the library's own events (matchy_scanner_get_unescape_timing), the call by the wall clock. Medians of --reps.
  escape-free   nginx-style log (tools/synth, config c2), under PERCENT and under JSON: every tile takes the copy path
  url-heavy     the url-heavy shape with its query strings percent-encoded (urllib.parse.quote), under PERCENT
  jsonl-app     the jsonl-app shape, every line nested as the string of a "message" field (\\" and \\\\), under JSON
The text of every input is compared once with what the construction says it is. Beside the figures stand those of the UTF-16 pass
(profiles/utf16_timing.txt), which has the same three steps on the same tiles. For the escape-free input the share of the HBM
bandwidth (--hbm-gbs) is given for two reads and one write of the batch.

    python tools/unescape_timing.py [--reps R] [--mib N] [--out FILE]"""
import argparse
import os
import re
import statistics
import sys
import time
import urllib.parse
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_inputs(mib):
    """[(name, modes, raw bytes, decoded bytes)]"""
    import matchy_amd as M
    from tools import synth
    cfg = synth.config("c2")
    n = mib << 20
    plain = synth.make_log(cfg, 0, n // 190)
    assert b"%" not in plain and b"\\" not in plain
    urls = synth.make_log(cfg, 0, n // 230, shape="url-heavy")
    enc = re.sub(rb"\?[^ \"\n]*", lambda m: b"?" + urllib.parse.quote(m.group()[1:], safe="=&").encode(), urls)
    assert b"%0A" not in enc and b"%0a" not in enc and urllib.parse.unquote_to_bytes(enc) == urls
    js = synth.make_log(cfg, 0, n // 330, shape="jsonl-app")
    assert js.endswith(b"\n")
    inner = js.replace(b"\\", b"\\\\").replace(b'"', b'\\"')
    nested = b'{"message":"' + inner[:-1].replace(b"\n", b'"}\n{"message":"') + b'"}\n'
    # an escaped backslash decodes to one, so the text is the line as it was, inside the field; the generator writes no escape for LF
    assert b"\\n" not in js and b"\\u000a" not in js.lower()
    flat = b'{"message":"' + js[:-1].replace(b"\n", b'"}\n{"message":"') + b'"}\n'
    if b"\\" in js:   # escapes of the log itself are decoded once more than they were encoded: take the reference's word for those lines
        sys.path.insert(0, str(ROOT / "tests"))
        import unescape_cases as U
        flat = U.reference(nested, U.JSON)[0]
    P, J = M.UNESCAPE_PERCENT, M.UNESCAPE_JSON
    return cfg, [("escape-free, PERCENT", P, plain, plain), ("escape-free, JSON", J, plain, plain), ("url-heavy, query strings percent-encoded, PERCENT", P, enc, urls),
                 ("jsonl-app nested in a message field, JSON", J, nested, flat)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth of the device in GB/s (MI355X: 8 TB/s)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "unescape_timing.txt"))
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import matchy_amd as M
    from tools import synth
    out("tools/unescape_timing.py --reps %d --mib %d" % (a.reps, a.mib))
    cfg, inputs = make_inputs(a.mib)
    db = M.Database(synth.build_db(cfg))
    sc = M.Scanner(db)
    med = statistics.median
    for name, modes, raw, want in inputs:
        dev = torch.empty(len(raw) + 64, dtype=torch.uint8, device="cuda")
        dev[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        torch.cuda.synchronize()
        r = sc.scan_escaped(dev.data_ptr(), modes, want_text=True, fetch_mode=0, nbytes=len(raw))   # buffers grow here; the text is checked once
        u = r.unescaped()
        assert u["text"] == want, name
        counters = (u["escapes"], u["replaced"], u["lf_escapes"])
        hits = r.n_hits
        r.close()
        steps, walls = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = sc.scan_escaped(dev.data_ptr(), modes, fetch_mode=0, nbytes=len(raw))
            walls.append((time.perf_counter() - t0) * 1e3)
            assert r.unescaped()["text_len"] == len(want) and r.n_hits == hits
            r.close()
            steps.append(sc.unescape_timing_ms())
        count, prefix, write = (med(s[k] for s in steps) for k in range(3))
        out("%s: %d bytes -> %d bytes, %d escapes, %d hits; milliseconds, median of %d" % (name, len(raw), len(want), counters[0], hits, a.reps))
        out("  count  %8.3f  (%.0f GB/s of input)" % (count, len(raw) / count / 1e6))
        out("  prefix %8.3f" % prefix)
        out("  write  %8.3f  (%.0f GB/s of input + output)" % (write, (len(raw) + len(want)) / write / 1e6))
        total = count + prefix + write
        out("  count + prefix + write %8.3f" % total)
        if raw is want:
            gbs = (2 * len(raw) + len(want)) / total / 1e6
            out("  two reads and one write of the batch in that time: %.0f GB/s = %.2f of %.0f GB/s" % (gbs, gbs / a.hbm_gbs, a.hbm_gbs))
        out("  decode + scan + fetch, wall clock of the call %8.3f" % med(walls))
        del dev
    out("the UTF-16 pass (profiles/utf16_timing.txt), the same three steps on the same tiles, 510610654 bytes -> 255305327 bytes:")
    out("  count     0.109  (4676 GB/s of input)   prefix    0.015   write     0.172  (4455 GB/s of input + output)")
    sc.close(); db.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
