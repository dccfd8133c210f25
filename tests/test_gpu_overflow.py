"""GPU: every work list overflowed BY NAME on a fresh scanner, through every entry that reaches it, and the regrow-and-rescan path
behind it (Scanner::fetch, Scanner::each_list).

The kernels count past a list's capacity without writing; fetch() grows every list that is over to its counted demand and runs the scan
again. With MATCHY_AMD_TRACE set fetch() names each list that was over, with demand and capacity:

    [matchy_amd] work buffers overflow (attempt 0): regrow and rescan: cands_a 60416>20000 final_ 20000>5000

(`name[k]` for slice k > 0 of a sliced scan). The scans run in child processes with the variable set, one at a time, each under its own
time limit. For every input the parent first checks ON THE CPU, from the oracle's result, that the demand exceeds the initial capacity
(the formulas of Work::ensure / slice_params / setup_spill, repeated in `initial_caps`; the capacities the trace prints must be these).
Per entry, on a new scanner:
  1. the dense batch: the trace names the intended lists; counters and the complete hit set equal the oracle's
  2. the same batch again: no overflow line (the demand was exact and the regrown lists suffice)
  3. a sparse ordinary batch (tools.synth log): equals the oracle. The grown lists still hold the dense batch's entries, so the
     consumers must read min(counter, capacity) slots of THIS scan and skip the sentinels. It may regrow lists the dense batch
     left small; only its result is checked.
  4. for the first entry, the same construction with a tenth more entries: it stays inside the headroom of the regrown lists
`attempt` in the trace is the number of regrows so far.
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ANCHOR_CHUNK = 1024


@pytest.fixture(scope="module")
def M():
    import matchy_amd
    matchy_amd.lib()
    return matchy_amd


def initial_caps(length):
    """Capacities of a fresh scanner's lists for a batch (or slice) of `length` bytes."""
    want_c = max(4096, length // 24)
    want_r = max(1024, length // 256)
    want_h = max(1024, want_c // 4)
    dom = -(-max(8192, length // 96) // ANCHOR_CHUNK) * ANCHOR_CHUNK
    return dict(cands=want_c, cands_a=want_c, cands_m=want_c // 8, cands_r=want_r, cands_d=want_r, rare=want_r, rare_dom=want_r, tok=want_r,
                heavy=want_r, dom_list=dom, hits=want_h, ids=want_h, glob_work=want_c // 8, glob_work_d=want_c // 8, spill=max(1024, want_c // 256),
                final_=want_h, final_ids_=2 * want_h, c4_=want_h)


# ------------------------------------------------------------------------------------------------ inputs
# A recipe gives (database entries, dense text). Everything is deterministic: parent and child build the same bytes.
SUFFIX = "example.com"


def _suffix_globs(n_sets):
    """Globs that all match `<label>.example.com`: '*' + every tail of the suffix, then the same behind '?*', '*?', 'n*' ...: 11 per set."""
    heads = ["*", "?*", "*?", "n*", "*.", "n*."][:n_sets]
    out = []
    for h in heads:
        for k in range(len(SUFFIX)):
            out.append(h + SUFFIX[k:])
    return out


def r_v4_dense(n=60000):
    text = b"".join(b"%d.%d.%d.%d " % (1 + i % 9, i % 10, (i // 10) % 10, (i // 100) % 10) for i in range(n))
    return [("0.0.0.0/1", {"h": 0}), ("128.0.0.0/1", {"h": 1})], text


def r_v4_sparse(n=60000):
    quads = ["1.1.1.1", "2.2.2.2", "3.3.3.3", "4.4.4.4"]
    text = b"".join(quads[i % 4].encode() + b" " for i in range(n))
    return [(q + "/32", {"q": q}) for q in quads], text


def r_domains(n=40000):
    names = ["a%d.io" % i for i in range(n)]
    return [(nm, {"k": i}) for i, nm in enumerate(names) if i % 2 == 0], (" ".join(names) + "\n").encode()


def r_misc(n=20000):
    # IPv6 and e-mail anchors (rare), e-mail keys for half; a database without globs: forked scans give these lists a stream of their own
    parts, ents = [], [("2001:db8::/32", {"net": "doc"})]
    for i in range(n):
        parts.append("2001:db8::%x u%d@a.co" % (i + 1, i))
        if i % 2 == 0:
            ents.append(("u%d@a.co" % i, {"u": i}))
    return ents, (" ".join(parts) + "\n").encode()


def r_heavy(n=6000):
    # Ethereum-shaped tokens (the heavy validators' list), every one a key
    toks = ["0x%040x" % (0xabcdef0123456789abcdef0000000000 + i * 7919) for i in range(n)]
    return [(t, {"e": i}) for i, t in enumerate(toks)], (" ".join(toks) + "\n").encode()


def r_hashes(n=20000):
    toks = ["%032x" % (0x5d41402abc4b2a76b9719d911017c592 + i * 104729) for i in range(n)]
    return [(t, {"h": i}) for i, t in enumerate(toks) if i % 2 == 0], (" ".join(toks) + "\n").encode()


def r_rare_dom(n=8000):
    # names k_validate_dom hands to the general walk: non-ASCII and longer than 64 bytes; every one a key
    names = ["ünï-çödé" * 5 + "%d.example.com" % i for i in range(n)]
    return [(nm, {"k": i}) for i, nm in enumerate(names)], (" ".join(names) + "\n").encode()


def r_globs20(n=30000):
    # every name passes the AC prefilter and matches 22 globs
    ents = [(g, {"g": i}) for i, g in enumerate(_suffix_globs(2))]
    return ents, (" ".join("n%d.%s" % (i, SUFFIX) for i in range(n)) + "\n").encode()


def r_spill(n=3000):
    # more than 1024 names that match more than 32 suffix globs each (beyond a lane's id storage: the spill pass)
    ents = [(g, {"g": i}) for i, g in enumerate(_suffix_globs(4))]
    return ents, (" ".join("n%d.%s" % (i, SUFFIX) for i in range(n)) + "\n").encode()


def r_cascade(n=60000):
    # ~1 MB of distinct short names, each matching 36 globs: every stage of the chain is far over its initial capacity
    ents = [(g, {"g": i}) for i, g in enumerate(_suffix_globs(4))]
    return ents, (" ".join("n%d.%s" % (i, SUFFIX) for i in range(n)) + "\n").encode()


def r_last_third(n=30000):
    # sparse in the first two thirds, dense IPv4 in the last: with three slices exactly one of them overflows
    ents, dense = r_v4_dense(n)
    filler = (b"x" * 63 + b"\n") * (2 * len(dense) // 64)
    return ents, filler + dense


RECIPES = dict(v4_dense=r_v4_dense, v4_sparse=r_v4_sparse, domains=r_domains, misc=r_misc, heavy=r_heavy, hashes=r_hashes, rare_dom=r_rare_dom,
               globs20=r_globs20, spill=r_spill, cascade=r_cascade, last_third=r_last_third)


def _padded(text, length):
    assert len(text) < length
    rest = length - len(text)
    return text + (b"x" * 63 + b"\n") * (rest // 64) + b"x" * (rest % 64)


def sweep_input(which, step):
    """One size of a sweep: `n` entries for a list whose capacity is pinned by padding the batch to a fixed length."""
    factor = (0.90, 0.93, 0.955, 0.97, 0.985, 0.995, 1.0, 1.004, 1.013, 1.03, 1.06, 1.10)[step]
    length = {"cands_a": 480_000, "dom_list": 1_572_864, "tok": 1_048_576, "final_": 480_000}[which]
    cap = initial_caps(length)[which]
    # the DEMAND is swept, and the demand of a chunked list is its entries plus what the waves leave unused of their last chunks: the domain
    # list is reserved in chunks of 1024 slots by the few waves a batch of this length gets (the trace shows ~4000 slots of padding, half a
    # chunk per wave), so its entry counts start that much lower; the other three lists are padded by a few per cent at most
    n = int((cap - (4096 if which == "dom_list" else 0)) * factor)
    if which == "cands_a":
        ents, text = r_v4_dense(n)
    elif which == "dom_list":
        ents, text = [("a1.io", {"k": 1})], (" ".join("a%d.io" % i for i in range(n)) + "\n").encode()
    elif which == "tok":
        ents, text = r_hashes(n)
        ents = ents[:10]
    else:   # final_: every name a literal key; cands (20 000 slots) holds them, final_ (5 000) is swept
        ents = [("a%d.io" % i, {"k": i}) for i in range(n)]
        text = (" ".join("a%d.io" % i for i in range(n)) + "\n").encode()
    return ents, _padded(text, length), cap, n


def build_blob(M, ents):
    b = M.DatabaseBuilder(build_epoch=1)
    for k, v in ents:
        b.add_entry(k, v)
    blob = b.build()
    b.close()
    return blob


# ------------------------------------------------------------------------------------------------ the child
CHILD = r"""
import ctypes, sys
sys.path[:0] = [%r, %r]
import matchy_amd as M
from oracle import oracle as orc
from tools import synth
import test_gpu_overflow as T
orc.build()
hip = ctypes.CDLL("libamdhip64.so")
KEY = lambda h: (h["start"], h["end"], h["type"], h["kind"])

def upload(text):
    d = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(len(text) + 64)) == 0
    assert hip.hipMemcpy(d, text, ctypes.c_size_t(len(text)), 1) == 0
    return d

def run(sc, how, d, text):
    kind, mode = how.split(":")
    mode = int(mode)
    if kind == "scan":
        return sc.scan(text)
    if kind == "sliced":
        sc.set_slices(3)
    if kind == "submitted":
        sc.submit_device(d.value, len(text), fetch_mode=mode)
        return sc.wait()
    return sc.scan_device(d.value, len(text), fetch_mode=mode)

def check(r, want, st, tag):
    assert (r.lines, r.candidates, r.n_hits) == (st.lines, st.candidates, len(want)), (tag, r.lines, r.candidates, r.n_hits, st.lines, st.candidates, len(want))
    got = sorted(r.hits(), key=KEY)
    assert got == want, tag
    r.close()

def mark(s):
    sys.stderr.write("[case] " + s + "\n"); sys.stderr.flush()

def oracle_scan(blob, text):
    want, _, st = orc.Database(blob).scan(text, want_json=False)
    return sorted(want, key=KEY), st

what = sys.argv[1]
if what == "sweep":
    which = sys.argv[2]
    for step in range(12):
        ents, text, cap, n = T.sweep_input(which, step)
        blob = T.build_blob(M, ents)
        want, st = oracle_scan(blob, text)
        db = M.Database(blob); sc = M.Scanner(db); d = upload(text)
        mark("step%%d scan1" %% step)
        check(run(sc, "forked:3", d, text), want, st, step)
        hip.hipFree(d); sc.close(); db.close()
else:
    ents, text = T.RECIPES[what]()
    blob = T.build_blob(M, ents)
    want, st = oracle_scan(blob, text)
    cfg = synth.config("c1")
    sparse = synth.make_log(cfg, 0, 3000)
    want_s, st_s = oracle_scan(blob, sparse)
    d, ds = upload(text), upload(sparse)
    db = M.Database(blob)
    for how in sys.argv[2].split(","):
        sc = M.Scanner(db)
        mark(how + " scan1"); check(run(sc, how, d, text), want, st, how + " dense")
        mark(how + " scan2"); check(run(sc, how, d, text), want, st, how + " again")
        mark(how + " scan3"); check(run(sc, how, ds, sparse), want_s, st_s, how + " sparse")
        if how == sys.argv[2].split(",")[0] and how == T.ALL_ENTRIES.split(",")[0] and what in T.CASES:
            # the same construction with a tenth more entries (same database): within the headroom a regrow leaves
            fn = T.RECIPES[what]
            _, more = fn(fn.__defaults__[0] * 11 // 10)
            want_m, st_m = oracle_scan(blob, more)
            dm = upload(more)
            mark(how + " scan4"); check(run(sc, how, dm, more), want_m, st_m, how + " a tenth more")
            hip.hipFree(dm)
        sc.close()
    db.close()
print("OK")
""" % (str(ROOT), str(ROOT / "tests"))

_FAULTED = []   # a child that died of a signal or ran into its time limit: no further GPU work from this module


OVER = re.compile(r"work buffers overflow \(attempt (\d+)\): regrow and rescan:(.*)$")


def run_child(args, env_extra=None, timeout=300):
    """Runs one child; returns {marker: [(attempt, {list: (demand, capacity)})]} and the spill lines."""
    env = {k: v for k, v in os.environ.items() if k not in ("MATCHY_AMD_NO_FORK", "MATCHY_AMD_MIRROR_RECS")}
    env.update(MATCHY_AMD_TRACE="1", **(env_extra or {}))
    assert not _FAULTED, "an earlier child faulted or hung (%s): nothing more is started on the GPU" % _FAULTED
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, *args], env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _FAULTED.append((args, "time limit"))
        raise
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _FAULTED.append((args, p.returncode))
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-1000:] + p.stderr[-3000:]
    trace, cur = {}, None
    for line in p.stderr.splitlines():
        if line.startswith("[case] "):
            cur = line[7:]
            trace[cur] = []
            continue
        m = OVER.search(line)
        if m and cur is not None:
            lists = {}
            toks = m.group(2).split()
            for name, dc in zip(toks[0::2], toks[1::2]):
                dem, cap = dc.split(">")
                lists[name] = (int(dem), int(cap))
            trace[cur].append((int(m.group(1)), lists))
            print(cur, "attempt", m.group(1), m.group(2))
    return trace, p.stderr


def _named(name, recipe, how):
    return "c4_" if name == "final_" and how.endswith(":9") and recipe.startswith("v4_") else name


def first_attempt(events, name):
    """The first attempt whose overflow line names `name` (of any slice), or None."""
    for attempt, lists in events:
        for k in lists:
            if k.split("[")[0] == name:
                return attempt
    return None


def demands(oracle, M, recipe):
    """What the oracle says the dense batch of a recipe holds: lower bounds of the lists' demands (padding comes on top)."""
    ents, text = RECIPES[recipe]()
    blob = build_blob(M, ents)
    hits, _, st = oracle.Database(blob).scan(text, want_json=False)
    by_type = {}
    for t, s, e, v in oracle.extract(text):
        by_type[t] = by_type.get(t, 0) + 1
    hit_type = {}
    for h in hits:
        hit_type[h["type"]] = hit_type.get(h["type"], 0) + 1
    return dict(length=len(text), cand=by_type, hit=hit_type, n_hits=len(hits), n_ids=sum(len(h["ids"]) for h in hits),
                n_glob=sum(1 for h in hits if h["ids"]), n_over32=sum(1 for h in hits if len(h["ids"]) > 32))


ALL_ENTRIES = "scan:3,forked:3,forked:1,forked:9,sliced:3,submitted:9"


def schedule(how):
    """The schedule an entry runs: everything on one stream (host buffer, submit / wait, MATCHY_AMD_NO_FORK), forked, or sliced."""
    return {"scan": "one", "submitted": "one", "forked": "fork", "sliced": "slice"}[how.split(":")[0]]


# Which lists a recipe must overflow, and on which attempt (= regrows so far) the trace must name each for the first time, per schedule.
#
# The attempt follows from the chain of producers: a list whose producers all fit shows on attempt 0; a list behind one that was over
# is under-counted until that one has been regrown and shows one attempt later, unless what the cut producer let through was already
# too much for it (then it shows on both). A pair (lo, hi) is given where that second case depends on which entries the atomics let
# into the cut list. The schedules differ in the lists they use: on one stream every validator writes `cands`; a forked scan gives
# the tokens / IPv6 / e-mail candidates `cands_m`, k_rare's `cands_r` and the undecided domains `cands_d`, and runs the early glob
# pass (`glob_work_d`); a sliced scan has `cands_m` and `cands_r` but neither `cands_d` nor the early glob pass.
#
# `hits` (and `ids` outside the spill pass) cannot be overflowed by a scan: k_lookup packs its records straight into final_ /
# final_ids_ (LookupParams::direct); the raw hit list is written for single queries only (Scanner::lookup_one, one candidate).
# final_ stands for it: it has the same capacity formula. With compact records (fetch_mode 9) the IPv4 records go to c4_ instead of
# final_ (`_named`).
#
# recipe -> ({list: lower bound of its demand from the oracle's counts}, {schedule: {list: attempt}}, lists with headroom to check)
CASES = {
    "v4_dense": (lambda d: dict(cands_a=d["cand"]["IPv4"], final_=d["n_hits"], c4_=d["n_hits"]),
                 dict(one=dict(cands_a=0, final_=0), fork=dict(cands_a=0, final_=0), slice=dict(cands_a=0, final_=0)), ("cands_a",)),
    "v4_sparse": (lambda d: dict(final_=d["n_hits"], c4_=d["n_hits"]),
                  dict(one=dict(final_=0), fork=dict(final_=0), slice=dict(final_=0)), ("final_",)),
    "domains": (lambda d: dict(dom_list=d["cand"]["Domain"], cands=d["hit"]["Domain"], final_=d["n_hits"]),
                dict(one=dict(dom_list=0, cands=1, final_=1), fork=dict(dom_list=0, cands=1, final_=1),
                     slice=dict(dom_list=0, cands=1, final_=(0, 1))), ()),
    "misc": (lambda d: dict(rare=d["cand"]["IPv6"] + d["cand"]["Email"], cands=d["n_hits"], cands_m=d["n_hits"], final_=d["n_hits"]),
             dict(one=dict(rare=0, cands=1, final_=1), fork=dict(rare=0, cands_m=1, final_=2), slice=dict(rare=0, cands_m=(0, 1), final_=2)),
             ("rare",)),
    "heavy": (lambda d: dict(tok=d["cand"]["Ethereum"], heavy=d["cand"]["Ethereum"], cands_r=d["n_hits"], final_=d["n_hits"]),
              dict(one=dict(tok=0, heavy=1, final_=2), fork=dict(tok=0, heavy=1, cands_r=2, final_=3), slice=dict(tok=0, heavy=1, cands_r=2, final_=3)),
              ("tok",)),
    "hashes": (lambda d: dict(tok=sum(d["cand"].values()), cands_m=d["n_hits"], final_=d["n_hits"]),
               dict(one=dict(tok=0, final_=1), fork=dict(tok=0, cands_m=1, final_=2), slice=dict(tok=0, cands_m=1, final_=2)), ("tok",)),
    "rare_dom": (lambda d: dict(rare_dom=d["cand"]["Domain"], cands_d=d["n_hits"], final_=d["n_hits"]),
                 # (the anchors of these long names also overflow dom_list, on attempt 0: rare_dom is one stage behind it)
                 dict(one=dict(rare_dom=1, final_=2), fork=dict(rare_dom=1, cands_d=2, final_=3), slice=dict(rare_dom=1, final_=2)), ()),
    "globs20": (lambda d: dict(dom_list=d["cand"]["Domain"], cands=d["n_hits"], glob_work=d["n_glob"], glob_work_d=d["n_glob"],
                               final_=d["n_hits"], final_ids_=d["n_ids"]),
                dict(one=dict(dom_list=0, glob_work=0, cands=1, final_=2, final_ids_=0),
                     fork=dict(dom_list=0, glob_work_d=0, cands=1, final_=2, final_ids_=0),
                     slice=dict(dom_list=0, glob_work=0, cands=1, final_=1, final_ids_=0)), ()),
    # the spill pass runs behind a scan that fits and appends to ids / final_ / final_ids_: they show one regrow behind spill
    "spill": (lambda d: dict(glob_work=d["n_glob"], glob_work_d=d["n_glob"], spill=d["n_over32"], ids=d["n_ids"], final_=d["n_hits"],
                             final_ids_=d["n_ids"]),
              dict(one=dict(glob_work=0, spill=1, ids=2, final_=2, final_ids_=2), fork=dict(glob_work_d=0, spill=1, ids=2, final_=2, final_ids_=2),
                   slice=dict(glob_work=0, spill=1, ids=2, final_ids_=2)), ()),
}


def check_attempts(recipe, how, ev, expect):
    for name, want in expect.items():
        got = first_attempt(ev, _named(name, recipe, how))
        lo, hi = want if isinstance(want, tuple) else (want, want)
        assert got is not None and lo <= got <= hi, (recipe, how, name, "attempt", got, "expected", want, ev)


@pytest.mark.parametrize("recipe", list(CASES))
def test_list_overflows_by_name(M, oracle, recipe):
    bounds, expect, headroom = CASES[recipe]
    d = demands(oracle, M, recipe)
    caps, caps3 = initial_caps(d["length"]), initial_caps(d["length"] // 3 + 8192)
    for name, low in bounds(d).items():
        print(recipe, name, "demand >=", low, "capacity", caps[name], "a slice's", caps3[name])
        assert low > caps[name], (recipe, name, low, caps[name])   # before the GPU is touched
    trace, err = run_child([recipe, ALL_ENTRIES])
    for how in ALL_ENTRIES.split(","):
        ev = trace[how + " scan1"]
        assert ev, (recipe, how, "no overflow line")
        check_attempts(recipe, how, ev, expect[schedule(how)])
        if schedule(how) != "slice":
            for name, (dem, cap) in ev[0][1].items():
                assert cap == caps[name], (recipe, how, name, cap, caps[name])   # the formulas above are the engine's
        assert trace[how + " scan2"] == [], (recipe, how, trace[how + " scan2"])   # the demand was exact, grown() sufficed
    # A regrow leaves headroom (grown(): a quarter more and 1024 slots), so that a batch a little denser than the last one does not
    # rescan: a tenth more entries of the same kind stay inside it. Asserted for lists whose first count was already complete (no
    # producer in front of them was over; a list behind one that was over is regrown from an under-count and may regrow again). The
    # domain list has a formula of its own and is left out.
    how0 = ALL_ENTRIES.split(",")[0]
    for name in headroom:
        assert first_attempt(trace[how0 + " scan4"], _named(name, recipe, how0)) is None, (recipe, name, trace[how0 + " scan4"])
    if recipe == "spill":
        assert "candidates to the spill pass" in err


def test_c4_overflows_with_compact_records(M, oracle):
    """fetch_mode 9 (compact IPv4 records): the dense IPv4 batch overflows c4_, whose capacity is final_'s, on attempt 0."""
    d = demands(oracle, M, "v4_dense")
    assert d["hit"]["IPv4"] > initial_caps(d["length"])["c4_"]
    trace, _ = run_child(["v4_dense", "forked:9,submitted:9,sliced:9"])
    for how in ("forked:9", "submitted:9", "sliced:9"):
        assert first_attempt(trace[how + " scan1"], "c4_") == 0, (how, trace[how + " scan1"])
        assert trace[how + " scan2"] == []


def test_one_slice_of_three_overflows(M, oracle):
    """Dense in its last third only: slice 2 overflows, slices 0 and 1 do not, and all three share final_ with it."""
    d = demands(oracle, M, "last_third")
    third = d["length"] // 3
    assert d["cand"]["IPv4"] > initial_caps(third + 8192)["cands_a"]
    # what the cut candidate list of slice 2 lets through is already more than the shared record array holds: both on attempt 0
    assert initial_caps(third)["cands_a"] - 2 * 1024 > 3 * initial_caps(third + 8192)["final_"]
    trace, _ = run_child(["last_third", "sliced:3,sliced:9"])
    for how in ("sliced:3", "sliced:9"):
        ev = trace[how + " scan1"]
        named = {k for _, lists in ev for k in lists}
        assert "cands_a[2]" in ev[0][1], (how, ev)
        assert not any(k.startswith("cands_a") and k != "cands_a[2]" for k in named), (how, ev)
        assert first_attempt(ev, "c4_" if how.endswith(":9") else "final_") == 0, (how, ev)
        assert trace[how + " scan2"] == []


@pytest.mark.parametrize("recipe", ["v4_dense", "domains", "hashes", "globs20"])
def test_overflow_on_one_stream(M, oracle, recipe):
    """MATCHY_AMD_NO_FORK=1: the device-resident entry on the caller's stream alone, one dense list of each kernel, on the attempts of
    the one-stream schedule."""
    trace, _ = run_child([recipe, "forked:3"], env_extra={"MATCHY_AMD_NO_FORK": "1"})
    check_attempts(recipe, "forked:3", trace["forked:3 scan1"], CASES[recipe][1]["one"])
    assert trace["forked:3 scan2"] == []


def test_small_mirror_with_a_list_overflow(M, oracle):
    """MATCHY_AMD_MIRROR_RECS=64: the pinned mirrors (records and compact records) hold 64 records, the batch has tens of thousands, in
    the same scan that overflows the candidate list and final_ / c4_: the copy path takes over, nothing is lost."""
    d = demands(oracle, M, "v4_dense")
    assert d["n_hits"] > 64 and d["hit"]["IPv4"] > 64   # neither mirror can hold the result
    trace, _ = run_child(["v4_dense", "forked:1,forked:9,sliced:9"], env_extra={"MATCHY_AMD_MIRROR_RECS": "64"})
    for how in ("forked:1", "forked:9", "sliced:9"):
        check_attempts("v4_dense", how, trace[how + " scan1"], CASES["v4_dense"][1][schedule(how)])
        assert trace[how + " scan2"] == []


@pytest.mark.parametrize("which", ["cands_a", "dom_list", "tok", "final_"])
def test_demand_swept_across_the_capacity(M, oracle, which):
    """A dozen sizes whose demand runs from about 0.9 to 1.1 times the list's initial capacity in uneven steps, so that chunks straddle
    the capacity at several alignments. final_ is swept in the place of hits, which a scan does not write (see CASES). Which sizes
    overflow depends on the per-wave padding and is not predicted: every size equals the oracle (checked in the child), some sizes
    overflow and some do not."""
    trace, _ = run_child(["sweep", which], timeout=600)
    over = []
    for step in range(12):
        ev = trace["step%d scan1" % step]
        if first_attempt(ev, which) is not None:
            over.append(step)
    print(which, "sizes that overflowed:", over)
    assert over, which
    assert len(over) < 12, which


MAX_REGROWS = 8   # Scanner::fetch: one regrow per stage of the longest chain of lists


def test_cascade_of_dense_stages(M, oracle):
    """A fresh scanner, the forked schedule, ~1 MB of distinct short names that each match 36 globs: dom_list, cands, glob_work_d,
    spill, ids and the final arrays are all far over their initial capacity, and while a list is over everything behind it
    under-counts. The scan must succeed and equal the oracle.

    fetch() used to give up when a scan was still over on its sixth pass through the loop, and the spill pass took one of those
    passes: this input overflowed on passes 0, 1, 2 and 4 (3 being the spill pass) and was accepted with nothing to spare; one more
    dense stage, as in a compact or sliced scan of the same names, would have been refused. fetch() now counts regrows only and
    allows MAX_REGROWS of them, one per stage of the longest chain of lists (every regrow settles at least the most upstream list
    that is over, whose count is exact).

    Measured on an MI355X: dom_list and spill on attempt 0, cands and glob_work_d on 1, spill again on 2 (its first count came from
    the cut candidate list), ids, final_ and final_ids_ behind the spill pass on 3: four regrows of the eight allowed."""
    d = demands(oracle, M, "cascade")
    caps = initial_caps(d["length"])
    assert d["cand"]["Domain"] > caps["dom_list"] and d["n_hits"] > caps["final_"] and d["n_hits"] > caps["cands"]
    assert d["n_ids"] > caps["ids"] and d["n_over32"] > caps["spill"] and d["n_glob"] > caps["glob_work_d"] and d["n_ids"] > caps["final_ids_"]
    trace, _ = run_child(["cascade", "forked:3"], timeout=600)
    ev = trace["forked:3 scan1"]
    print("cascade attempts:", [a for a, _ in ev])
    check_attempts("cascade", "forked:3", ev, dict(dom_list=0, spill=0, cands=1, glob_work_d=1, ids=3, final_=3, final_ids_=3))
    assert ev[-1][0] == 3 and ev[-1][0] < MAX_REGROWS, ev
    assert any("spill" in lists for a, lists in ev if a == 2), ev
    assert trace["forked:3 scan2"] == []
