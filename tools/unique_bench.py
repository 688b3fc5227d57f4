#!/usr/bin/env python3
"""Times of adlhip_unique_typed next to the sorts it is built on, and next to torch.unique on the same keys.

    python tools/unique_bench.py [n = 64 Mi] [--reps 5] [--out profiles/unique_bench_64m.txt]

Per distribution -- few keys (256 distinct int32 values), many keys (int32, all distinct), float32 standard normal -- the median of
`reps` timed runs after one warm-up of
  unique (keys path)    adlhip_unique_typed with counts: copy + adlhip_sort_keys_typed + the run stage
  sort keys             adlhip_sort_keys_typed alone on the same handle: the floor the run stage adds to
  unique (index path)   adlhip_unique_typed with counts and inverse: adlhip_argsort_typed + the run stage with the permutation
  argsort               adlhip_argsort_typed with keys out alone: the floor of the index path
  torch.unique          torch.unique(t, return_counts=True) and torch.unique(t, return_inverse=True, return_counts=True)
Library calls are timed with hipEvents on the handle's stream, torch with torch.cuda events; every output buffer is allocated before
the timed runs.  The library's results are compared with torch's before they are counted (the keys hold no NaN and no -0).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # before the HIP back-end is loaded: one HIP runtime per process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, Stopwatch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=1 << 26)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
n, reps = args.n, args.reps
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    if args.out:   # kept current: a run that is cut short leaves what it measured
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


d = DeviceUtils.allocate()
p = Pprims()
say("# unique_bench: n = %d (%.0f Mi) keys, median of %d timed runs per case after one warm-up; device %s" % (
    n, n / (1 << 20), reps, d.getDeviceName()))


def timed(run, before=None):
    times = []
    for r in range(reps + 1):
        if before:
            before()
        DeviceUtils.waitForCompletion(d)
        sw = Stopwatch(d)
        sw.start()
        run()
        sw.stop()
        DeviceUtils.waitForCompletion(d)
        if r:
            times.append(sw.getMs())
    return statistics.median(times), times


def timed_torch(run):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
        del out
    return statistics.median(times), times


def keys_of(dist):
    rng = np.random.default_rng(7)
    if dist == "few":
        return (rng.integers(0, 256, size=n).astype(np.int32) * np.int32(7919) - np.int32(1 << 20)).astype(np.int32)
    if dist == "many":
        return rng.permutation(n).astype(np.int32)
    x = rng.standard_normal(n).astype(np.float32)
    x[x == 0] = 1.0   # no -0 (and no +0 either)
    return x


def row(label, ms, ts, floor=None):
    extra = "" if floor is None else "  (%.3f ms over %s)" % (ms - floor[1], floor[0])
    say("    %-34s %9.3f ms  %7.2f Gkeys/s  [%s]%s" % (label, ms, n / ms / 1e6, " ".join("%.3f" % t for t in ts), extra))


for dist, title in (("few", "few keys: int32, 256 distinct values"), ("many", "many keys: int32, all distinct"),
                    ("normal", "float32, standard normal")):
    host = keys_of(dist)
    dtype = host.dtype
    keys = Buffer(d, n, dtype)
    keys.write(host)
    scratch = Buffer(d, n, dtype)
    sorted_out = Buffer(d, n, dtype)
    uniq = Buffer(d, n, dtype)
    counts = Buffer(d, n, np.uint32)
    inverse = Buffer(d, n, np.uint32)
    index = Buffer(d, n, np.uint32)
    count = Buffer(d, 1, np.uint32)
    DeviceUtils.waitForCompletion(d)
    t = torch.from_numpy(host).cuda()
    say()
    say("## %s" % title)

    want_u, want_c = torch.unique(t, return_counts=True)
    r_want = want_u.numel()
    u_ms, u_ts = timed(lambda: p.unique(d, keys, n, counts=counts, uniqueOut=uniq, countOut=count))
    r = int(count.toHost()[0])
    ok = r == r_want and np.array_equal(uniq.toHost()[:r], want_u.cpu().numpy()) and \
        np.array_equal(counts.toHost()[:r].astype(np.int64), want_c.cpu().numpy())
    s_ms, s_ts = timed(lambda: p.sortKeys(d, scratch, n), before=lambda: p.copy(d, scratch, keys, n))
    row("sort keys", s_ms, s_ts)
    row("unique, counts (keys path)", u_ms, u_ts, ("sort keys", s_ms))
    say("    %d distinct keys  %s" % (r, "OK" if ok else "MISMATCH"))

    want_u, want_i, want_c = torch.unique(t, return_inverse=True, return_counts=True)
    x_ms, x_ts = timed(lambda: p.unique(d, keys, n, counts=counts, inverse=inverse, uniqueOut=uniq, countOut=count))
    r = int(count.toHost()[0])
    ok = r == r_want and np.array_equal(uniq.toHost()[:r], want_u.cpu().numpy()) and \
        np.array_equal(counts.toHost()[:r].astype(np.int64), want_c.cpu().numpy()) and \
        np.array_equal(inverse.toHost().astype(np.int64), want_i.cpu().numpy())
    del want_u, want_i, want_c
    a_ms, a_ts = timed(lambda: p.argsort(d, keys, n, keysOut=sorted_out, indexOut=index))
    row("argsort + keys out", a_ms, a_ts)
    row("unique, counts, inverse (index path)", x_ms, x_ts, ("argsort", a_ms))
    say("    %s" % ("OK" if ok else "MISMATCH"))

    t_ms, t_ts = timed_torch(lambda: torch.unique(t, return_counts=True))
    row("torch.unique, counts", t_ms, t_ts)
    t_ms, t_ts = timed_torch(lambda: torch.unique(t, return_inverse=True, return_counts=True))
    row("torch.unique, counts, inverse", t_ms, t_ts)
    del t
    torch.cuda.empty_cache()
    for b in (keys, scratch, sorted_out, uniq, counts, inverse, index, count):
        b.release()

p.close()
DeviceUtils.deallocate(d)
