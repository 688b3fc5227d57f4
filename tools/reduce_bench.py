#!/usr/bin/env python3
"""Times of adlhip_reduce_runs and adlhip_reduce_by_key_typed next to the calls they are built on, and next to torch on the same tensors.

    python tools/reduce_bench.py [n = 64 Mi] [--reps 5] [--out profiles/reduce_by_key_bench_64m.txt]

Per (key, value) type -- (int32, float32) and (int64, float64) -- and key distribution -- few keys (256 distinct values), many keys (all
distinct), float32 standard normal keys (with the 4-byte pair only) -- the median of `reps` timed runs after one warm-up of
  read both arrays     adlhip_probe_read over the keys, then over the values: what one pass over the input costs
  run-length encode    adlhip_run_length_encode on the sorted keys: the run stage without values
  reduce runs          adlhip_reduce_runs (sum) on the sorted keys and their values
  sort pairs           adlhip_sort_pairs_typed alone on copies of the unsorted arrays (the copies are not timed)
  reduce by key        adlhip_reduce_by_key_typed (sum) on the unsorted arrays
  torch                torch.unique(keys, return_inverse=True) followed by zeros(R).index_add_(0, inverse, values)
Library calls are timed with hipEvents on the handle's stream, torch with torch.cuda events; every output buffer is allocated before
the timed runs.  The values are small integers stored as floats, so that sums are exact in every order, and the library's keys and sums
are compared with torch's before they are counted (the keys hold no NaN and no -0).
"""
import argparse
import ctypes
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
lib = _lib.load()
say("# reduce_bench: n = %d (%.0f Mi) (key, value) pairs, median of %d timed runs per case after one warm-up; device %s" % (
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


def keys_of(dist, kdt):
    rng = np.random.default_rng(7)
    if dist == "few":
        return (rng.integers(0, 256, size=n).astype(kdt) * kdt(7919) - kdt(1 << 20)).astype(kdt)
    if dist == "many":
        return rng.permutation(n).astype(kdt)
    x = rng.standard_normal(n).astype(np.float32)
    x[x == 0] = 1.0   # no -0 (and no +0 either)
    return x


def row(label, ms, ts, floor=None):
    extra = "" if floor is None else "  (%.3f ms over %s)" % (ms - floor[1], floor[0])
    say("    %-34s %9.3f ms  %7.2f Gpairs/s  [%s]%s" % (label, ms, n / ms / 1e6, " ".join("%.3f" % t for t in ts), extra))


CASES = [(np.int32, np.float32, "few", "int32 keys, 256 distinct values; float32 values"),
         (np.int32, np.float32, "many", "int32 keys, all distinct; float32 values"),
         (np.float32, np.float32, "normal", "float32 keys, standard normal; float32 values"),
         (np.int64, np.float64, "few", "int64 keys, 256 distinct values; float64 values"),
         (np.int64, np.float64, "many", "int64 keys, all distinct; float64 values")]

for kdt, vdt, dist, title in CASES:
    host_k = keys_of(dist, kdt)
    host_v = np.random.default_rng(8).integers(-8, 9, size=n).astype(vdt)      # |sum| <= 8 n: exact in float32 up to n = 2 Mi per key
    if dist == "few" and vdt == np.float32:
        host_v = np.random.default_rng(8).integers(-1, 2, size=n).astype(vdt)  # n / 256 elements per key: keep |sum| below 2^24
    kdtype, vdtype = host_k.dtype, host_v.dtype
    keys, vals = Buffer(d, n, kdtype), Buffer(d, n, vdtype)
    keys.write(host_k)
    vals.write(host_v)
    skeys, svals = Buffer(d, n, kdtype), Buffer(d, n, vdtype)
    uniq, red = Buffer(d, n, kdtype), Buffer(d, n, vdtype)
    count = Buffer(d, 1, np.uint32)
    sink = Buffer(d, 2, np.uint32)
    DeviceUtils.waitForCompletion(d)
    tk, tv = torch.from_numpy(host_k).cuda(), torch.from_numpy(host_v).cuda()
    say()
    say("## %s" % title)

    want_u, inv = torch.unique(tk, return_inverse=True)
    want_s = torch.zeros(want_u.numel(), dtype=tv.dtype, device="cuda").index_add_(0, inv, tv)
    r_want = want_u.numel()
    want_u, want_s = want_u.cpu().numpy(), want_s.cpu().numpy()
    del inv

    # sorted input for the run stages
    p.copy(d, skeys, keys, n)
    p.copy(d, svals, vals, n)
    p.sortPairs(d, skeys, svals, n)
    kb, vb = n * kdtype.itemsize, n * vdtype.itemsize
    f_ms, f_ts = timed(lambda: (check(lib.adlhip_probe_read(d._h, skeys.ptr(), kb, sink.ptr()), "probe_read"),
                                check(lib.adlhip_probe_read(d._h, svals.ptr(), vb, sink.ptr()), "probe_read")))
    row("read both arrays", f_ms, f_ts)
    e_ms, e_ts = timed(lambda: p.runLengthEncode(d, skeys, n, uniqueOut=uniq, countOut=count))
    row("run-length encode", e_ms, e_ts)
    rr_ms, rr_ts = timed(lambda: p.reduceRuns(d, skeys, svals, n, uniqueOut=uniq, reducedOut=red, countOut=count))
    r = int(count.toHost()[0])
    ok = r == r_want and np.array_equal(uniq.toHost()[:r], want_u) and np.array_equal(red.toHost()[:r], want_s)
    row("reduce runs (sum)", rr_ms, rr_ts, ("run-length encode", e_ms))
    say("    %d runs  %s" % (r, "OK" if ok else "MISMATCH"))

    def reset():
        p.copy(d, skeys, keys, n)
        p.copy(d, svals, vals, n)
    s_ms, s_ts = timed(lambda: p.sortPairs(d, skeys, svals, n), before=reset)
    row("sort pairs", s_ms, s_ts)
    b_ms, b_ts = timed(lambda: p.reduceByKey(d, keys, vals, n, uniqueOut=uniq, reducedOut=red, countOut=count))
    r = int(count.toHost()[0])
    ok = r == r_want and np.array_equal(uniq.toHost()[:r], want_u) and np.array_equal(red.toHost()[:r], want_s)
    row("reduce by key (sum)", b_ms, b_ts, ("sort pairs", s_ms))
    say("    %d distinct keys  %s" % (r, "OK" if ok else "MISMATCH"))

    def torch_way():
        u, i = torch.unique(tk, return_inverse=True)
        return u, torch.zeros(u.numel(), dtype=tv.dtype, device="cuda").index_add_(0, i, tv)
    t_ms, t_ts = timed_torch(torch_way)
    row("torch.unique + index_add_", t_ms, t_ts)
    del tk, tv
    torch.cuda.empty_cache()
    for b in (keys, vals, skeys, svals, uniq, red, count, sink):
        b.release()

p.close()
DeviceUtils.deallocate(d)
