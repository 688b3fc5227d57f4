#!/usr/bin/env python3
"""Times of adlhip_scan_typed and adlhip_scan_by_key next to the calls they are compared with, and next to torch on the same tensors.

    python tools/scan_bench.py [n = 64 Mi] [--reps 15] [--inner 8] [--out profiles/scan_bench_64m.txt]

Plain inclusive sums of uint32, float32, int64 and float64 values, and sums by key of (int32 key, float32 value) pairs with 256 distinct
keys (sorted: 256 runs), all keys distinct, and one run.  Each next to
  copy probe           adlhip_probe_copy of the n values: one read and one write, the floor of anything that writes n results
  u32 scan             adlhip_exclusive_scan_u32 (uint32 values only): the reference's scan, which keeps its own kernels
  reduce runs          adlhip_reduce_runs (sum) on the same keys and values (by key only): the same two reading launches, no n-element write
  torch.cumsum         torch.cumsum(values, 0, dtype=values.dtype); torch has no by-key form, so by key it is the plain cumsum of the values
The bytes-moved model: a plain scan reads the values twice and writes them once, 1.5 x the copy probe's traffic; a scan by key moves
what reduce runs moves (keys and values read twice) plus one write of the values.

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round, and the median counts.  Library calls are timed with hipEvents on the handle's stream, torch with
torch.cuda events; every buffer is allocated before the timed runs.  The values are -1, 0 and 1, so that float sums are exact in every
order, and the library's result is compared with torch's before it is counted.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # before the HIP back-end is loaded: one HIP runtime per process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, Stopwatch, _lib  # noqa: E402
from oclradixsort_amd._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=1 << 26)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--inner", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
n, reps, inner = args.n, args.reps, args.inner
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    if args.out:   # kept current: a run that is cut short leaves what it measured
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


d = DeviceUtils.allocate()
p = Pprims()
lib = _lib.load()
say("# scan_bench: n = %d (%.0f Mi) elements; per contender the median of %d samples of %d calls each, taken in turns after one warm-up "
    "round; device %s" % (n, n / (1 << 20), reps, inner, d.getDeviceName()))


def sample_lib(run):
    DeviceUtils.waitForCompletion(d)
    sw = Stopwatch(d)
    sw.start()
    for _ in range(inner):
        run()
    sw.stop()
    DeviceUtils.waitForCompletion(d)
    return sw.getMs() / inner


def sample_torch(run):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = run()
        del out
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def in_turns(contenders):
    """contenders: [(label, sampler, run)] -> {label: (median, samples)}"""
    times = {label: [] for label, _, _ in contenders}
    for r in range(reps + 1):
        for label, sampler, run in contenders:
            t = sampler(run)
            if r:
                times[label].append(t)
    return {label: (statistics.median(ts), ts) for label, ts in times.items()}


def report(res, order, moved):
    """moved: {label: bytes the call has to move}"""
    for label in order:
        ms, ts = res[label]
        say("    %-28s %8.3f ms  %6.2f Gelem/s  %6.0f GB/s of its model  (min %.3f, max %.3f)" % (
            label, ms, n / ms / 1e6, moved[label] / ms / 1e6, min(ts), max(ts)))


PLAIN = [(np.uint32, "uint32"), (np.float32, "float32"), (np.int64, "int64"), (np.float64, "float64")]
for vdt, name in PLAIN:
    host_v = np.random.default_rng(8).integers(-1, 2, size=n).astype(np.int64).astype(vdt)   # (uint32: 0xffffffff, 0, 1 -- sums wrap)
    vals, out = Buffer(d, n, vdt), Buffer(d, n, vdt)
    vals.write(host_v)
    DeviceUtils.waitForCompletion(d)
    tdt = {"uint32": torch.int32, "float32": torch.float32, "int64": torch.int64, "float64": torch.float64}[name]
    tv = torch.from_numpy(host_v.view(np.int32) if name == "uint32" else host_v).cuda()
    say()
    say("## plain inclusive sum, %s values" % name)
    p.scanTyped(d, out, vals, n)
    want = torch.cumsum(tv, 0, dtype=tdt).cpu().numpy()
    ok = np.array_equal(out.toHost().view(want.dtype), want)
    vb = n * np.dtype(vdt).itemsize
    contenders = [("scan typed (inclusive sum)", sample_lib, lambda: p.scanTyped(d, out, vals, n)),
                  ("copy probe", sample_lib, lambda: check(lib.adlhip_probe_copy(d._h, out.ptr(), vals.ptr(), vb), "probe_copy")),
                  ("torch.cumsum", sample_torch, lambda: torch.cumsum(tv, 0, dtype=tdt))]
    moved = {"scan typed (inclusive sum)": 3 * vb, "copy probe": 2 * vb, "torch.cumsum": 2 * vb}
    if name == "uint32":
        p.scan(d, out, vals, n)   # sizes its scratch outside the timed runs
        contenders.insert(2, ("u32 scan (exclusive)", sample_lib, lambda: p.scan(d, out, vals, n)))
        moved["u32 scan (exclusive)"] = 3 * vb
    res = in_turns(contenders)
    report(res, [c[0] for c in contenders], moved)
    say("    result %s;  scan / copy probe = %.2f (model 1.5);  scan / torch.cumsum = %.2f%s" % (
        "OK" if ok else "MISMATCH", res["scan typed (inclusive sum)"][0] / res["copy probe"][0],
        res["scan typed (inclusive sum)"][0] / res["torch.cumsum"][0],
        ";  scan / u32 scan = %.2f" % (res["scan typed (inclusive sum)"][0] / res["u32 scan (exclusive)"][0]) if name == "uint32" else ""))
    del tv
    torch.cuda.empty_cache()
    for b in (vals, out):
        b.release()

KEYED = [("256 distinct keys (256 runs)", lambda: np.sort(np.random.default_rng(7).integers(0, 256, size=n).astype(np.int32))),
         ("all keys distinct (n runs)", lambda: np.arange(n, dtype=np.int32)),
         ("one run", lambda: np.full(n, 42, dtype=np.int32))]
for title, make in KEYED:
    host_k = make()
    host_v = np.random.default_rng(8).integers(-1, 2, size=n).astype(np.float32)
    keys, vals, out = Buffer(d, n, np.int32), Buffer(d, n, np.float32), Buffer(d, n, np.float32)
    uniq, red, count = Buffer(d, n, np.int32), Buffer(d, n, np.float32), Buffer(d, 1, np.uint32)
    keys.write(host_k)
    vals.write(host_v)
    DeviceUtils.waitForCompletion(d)
    tk, tv = torch.from_numpy(host_k).cuda(), torch.from_numpy(host_v).cuda()
    say()
    say("## inclusive sum by key, int32 keys, float32 values: %s" % title)
    p.scanByKey(d, keys, out, vals, n)
    # torch has no by-key scan: the plain cumsum in float64 (exact here) minus what was carried into each run
    c = torch.cumsum(tv, 0, dtype=torch.float64)
    head = torch.ones(n, dtype=torch.bool, device="cuda")
    head[1:] = tk[1:] != tk[:-1]
    starts = torch.nonzero(head).flatten()
    seg = torch.cumsum(head, 0) - 1
    want = (c - (c - tv.double())[starts][seg]).float().cpu().numpy()
    ok = np.array_equal(out.toHost(), want)
    del c, head, starts, seg
    torch.cuda.empty_cache()
    p.reduceRuns(d, keys, vals, n, uniqueOut=uniq, reducedOut=red, countOut=count)   # sizes the scratch outside the timed runs
    kb, vb = n * 4, n * 4
    contenders = [("scan by key (inclusive sum)", sample_lib, lambda: p.scanByKey(d, keys, out, vals, n)),
                  ("reduce runs (sum)", sample_lib, lambda: p.reduceRuns(d, keys, vals, n, uniqueOut=uniq, reducedOut=red, countOut=count)),
                  ("copy probe (values)", sample_lib, lambda: check(lib.adlhip_probe_copy(d._h, out.ptr(), vals.ptr(), vb), "probe_copy")),
                  ("torch.cumsum (values, plain)", sample_torch, lambda: torch.cumsum(tv, 0))]
    runs = int(count.toHost()[0])
    moved = {"scan by key (inclusive sum)": 2 * (kb + vb) + vb, "reduce runs (sum)": 2 * (kb + vb) + runs * (4 + 4),
             "copy probe (values)": 2 * vb, "torch.cumsum (values, plain)": 2 * vb}
    res = in_turns(contenders)
    report(res, [c[0] for c in contenders], moved)
    s, r, cp = res["scan by key (inclusive sum)"][0], res["reduce runs (sum)"][0], res["copy probe (values)"][0]
    say("    result %s;  %d runs;  scan by key / (reduce runs + half a copy probe) = %.2f (model 1.0);  scan by key / reduce runs = %.2f;  "
        "scan by key / copy probe = %.2f" % ("OK" if ok else "MISMATCH", runs, s / (r + cp / 2), s / r, s / cp))
    del tk, tv
    torch.cuda.empty_cache()
    for b in (keys, vals, out, uniq, red, count):
        b.release()

p.close()
DeviceUtils.deallocate(d)
