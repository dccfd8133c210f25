"""Logs, the plain-Python model and the runners shared by tests/test_gpu_distinct.py and the child processes it starts (the
MATCHY_AMD_DISTINCT_* overrides and MATCHY_AMD_HOST_PIECE_BYTES are read when a handle / the library first needs them, so the cases
that set them run in a process of their own: `python tests/distinct_cases.py <case>` prints what the unique handle returned as JSON;
the parent, which has none of them set, computes the model)."""
import json
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HEX = "0123456789abcdef"
BTC = ["1A1zP1eP5QGefi2DMPTfTL5SLmv7DivfNa", "3Cbq7aT1tY8kMxWLbitaG7yT6bPbKChq64", "bc1qar0srrr7xfkvy5l643lydnw9re59gtzzwf5mdq"]
WORDS = ["GET", "status=200", "ok", "from", "to", "user", "-", "req", "id=7", "took", "12ms", "cache", "miss"]


def _hex(rng, n):
    return "".join(rng.choice(HEX) for _ in range(n))


def basic_texts(rng):
    """About 300 distinct candidate texts of all eight extractor classes, with pairs that differ only in letter case and a text
    that is a proper prefix of another."""
    xmr = json.loads((ROOT / "tests" / "golden" / "xmr_kat.json").read_text())["accept"][:4]
    t = ["a.example.com", "aa.example.com", "host1.example.com", "Host1.Example.com", "HOST1.example.com",
         "2001:db8::a", "2001:DB8::A", "2001:db8::1", "2001:db8:85a3::8a2e:370:7334",
         "alice@test.com", "Alice@test.com", "user+tag@example.com"]
    t += BTC + xmr
    t += ["%d.%d.%d.%d" % (rng.randrange(1, 224), rng.randrange(256), rng.randrange(256), rng.randrange(1, 255)) for _ in range(80)]
    t += ["2001:db8:%x::%x" % (rng.randrange(1, 0xFFFF), rng.randrange(1, 0xFFFF)) for _ in range(25)]
    t += ["user%d@mail%d.example.org" % (rng.randrange(1000), rng.randrange(20)) for _ in range(30)]
    t += ["host%d.srv%d.example.net" % (rng.randrange(1000), rng.randrange(30)) for _ in range(80)]
    for n in (32, 40, 64, 96, 128):
        for _ in range(8):
            h = _hex(rng, n)
            t += [h, h.upper()] if n == 32 else [h]
    t += ["0x" + _hex(rng, 40) for _ in range(10)]
    return list(dict.fromkeys(t))


def make_log(rng, texts, n_tokens, heavy=None, heavy_share=0.0):
    """Lines of one to three tokens between filler words; `heavy` takes heavy_share of the draws."""
    out, left = [], n_tokens
    while left > 0:
        k = min(left, rng.randrange(1, 4))
        parts = [rng.choice(WORDS)]
        for _ in range(k):
            tok = heavy if heavy is not None and rng.random() < heavy_share else rng.choice(texts)
            parts += [tok, rng.choice(WORDS)]
        parts += [rng.choice(WORDS) for _ in range(rng.randrange(6, 20))]
        out.append(" ".join(parts) + "\n")
        left -= k
    return "".join(out).encode()


def basic_log():
    rng = random.Random(20261018)
    return make_log(rng, basic_texts(rng), 4400, heavy="10.0.0.1", heavy_share=0.5)


def many_distinct_log(n_distinct, seed):
    rng = random.Random(seed)
    texts = ["n%d.z%d.example.com" % (i, i % 97) if i % 3 else "10.%d.%d.%d" % (i >> 16, (i >> 8) & 255, i & 255) for i in range(n_distinct)]
    toks = texts + [rng.choice(texts) for _ in range(n_distinct // 3)]
    rng.shuffle(toks)
    return "".join("%s %s %s\n" % (rng.choice(WORDS), t, rng.choice(WORDS)) for t in toks).encode()


def cut(data, n_chunks):
    """`data` in n_chunks pieces that end behind a newline."""
    cuts, step = [0], len(data) // n_chunks
    for k in range(1, n_chunks):
        cuts.append(data.index(b"\n", max(cuts[-1], k * step)) + 1)
    cuts.append(len(data))
    return [data[a:b] for a, b in zip(cuts, cuts[1:])]


def first_occurrences(items, data, seen):
    """The model: walk the extractor's output in order; an entry stays when its text data[start:end] is not in `seen` yet."""
    keep = []
    for it in items:
        text = data[it[1]:it[2]]
        if text not in seen:
            seen.add(text)
            keep.append(it)
    return keep


def run_chunks(chunks, unique):
    """One handle over the chunks: (items with offsets rebased to the concatenation, unique_count after every chunk)."""
    import matchy_amd as M
    ex = M.Extractor(M.EXTRACT_ALL, unique=unique)
    got, counts, base = [], [], 0
    for ch in chunks:
        got += [[t, s + base, e + base, v] for t, s, e, v in ex.extract_from_chunk(ch)]
        counts.append(ex.unique_count)
        base += len(ch)
    ex.close()
    return got, counts


def model_chunks(chunks):
    """The same handle class with unique off, filtered chunk after chunk by the model."""
    import matchy_amd as M
    ex = M.Extractor(M.EXTRACT_ALL)
    want, counts, base, seen = [], [], 0, set()
    for ch in chunks:
        items = ex.extract_from_chunk(ch)
        want += [[t, s + base, e + base, v] for t, s, e, v in first_occurrences(items, ch, seen)]
        counts.append(len(seen))
        base += len(ch)
    ex.close()
    return want, counts


CASES = {
    # name: (log, chunks)
    "pieces": lambda: (basic_log(), 1),
    "growth": lambda: (many_distinct_log(5000, 7), 4),
    "collide4": lambda: (many_distinct_log(500, 8), 2),
    "collide0": lambda: (many_distinct_log(64, 9), 2),
}


def main(name):
    data, n = CASES[name]()
    chunks = cut(data, n)
    got, got_counts = run_chunks(chunks, True)
    json.dump({"got": got, "got_counts": got_counts}, sys.stdout)


if __name__ == "__main__":
    main(sys.argv[1])
