#!/usr/bin/env python3
"""Times of adlhip_topk_typed next to the same result obtained by the full argsort, and next to one read of the keys.

    python tools/topk_bench.py [n = 64 Mi] [--reps 5] [--quick] [--out profiles/topk_bench_64m.txt]

Per (key type, order, distribution, k): device time (hipEvents around the call, median of `reps` runs after one warm-up) of
  select   adlhip_topk_typed with "topk.algo" = 1 (radix select + k-element finish)
  argsort  adlhip_argsort_typed with keys out -- how the first k were obtained before top-k existed; it does not depend on k and is
           measured once per (type, order, distribution), in the same run
their ratio, and for the selection the bytes of the key array divided by its time as a fraction of the read probe's rate
(adlhip_probe_read_ex, the better of plain and non-temporal loads, measured here on the same array): the floor is one read.
Distributions: uniform random bits (u), standard-normal floats (n, float types only), all keys equal (e).
Every selection result is compared with the first k entries of the argsort's result (indices and key bits) before it is counted.
--quick: f32 only, descending only.
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, Stopwatch, _lib  # noqa: E402
from oclradixsort_amd._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", type=int, default=1 << 26)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true")
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
say("# topk_bench: n = %d (%.0f Mi) keys, median of %d timed runs per case after one warm-up; device %s" % (
    n, n / (1 << 20), reps, d.getDeviceName()))
KS = [k for k in (1, 64, 4096, 64 << 10, 1 << 20, 8 << 20) if k <= n]


def timed(run):
    times = []
    for r in range(reps + 1):
        DeviceUtils.waitForCompletion(d)
        sw = Stopwatch(d)
        sw.start()
        run()
        sw.stop()
        DeviceUtils.waitForCompletion(d)
        if r:
            times.append(sw.getMs())
    return statistics.median(times), times


def read_rate(buf, nbytes):
    """GB/s of the read probe on this array, the better of its two variants"""
    sink = Buffer(d, 16, np.uint8)
    best = 0.0
    for hints in (0, 1):
        ms, _ = timed(lambda: check(lib.adlhip_probe_read_ex(d._h, buf.ptr(), nbytes, sink.ptr(), hints, 8), "probe_read_ex"))
        best = max(best, nbytes / ms / 1e6)
    sink.release()
    return best


def fill(buf, dtype, dist):
    w = np.dtype(dtype).itemsize
    if dist == "u":
        raw = Buffer(d, n * w // 4, np.uint32)
        raw.generate(n * w // 4, seed=2026)
        check(lib.adlhip_memcpy_d2d(d._h, buf.ptr(), raw.ptr(), n * w), "d2d")
        DeviceUtils.waitForCompletion(d)
        raw.release()
    elif dist == "n":
        buf.write(np.random.default_rng(7).standard_normal(n).astype(dtype))
    else:
        buf.write(np.full(n, 1.5 if np.dtype(dtype).kind == "f" else 12345, dtype=dtype))
    DeviceUtils.waitForCompletion(d)


TYPES = [("f32", np.float32)] if args.quick else [("f32", np.float32), ("i32", np.int32), ("f64", np.float64)]
ORDERS = [True] if args.quick else [True, False]
for name, dtype in TYPES:
    w = np.dtype(dtype).itemsize
    udt = np.uint32 if w == 4 else np.uint64
    keys = Buffer(d, n, dtype)
    full_k = Buffer(d, n, dtype)
    full_i = Buffer(d, n, np.uint32)
    out_k = Buffer(d, max(KS), dtype)
    out_i = Buffer(d, max(KS), np.uint32)
    for dist in ("u", "n", "e"):
        if dist == "n" and np.dtype(dtype).kind != "f":
            continue
        fill(keys, dtype, dist)
        rate = read_rate(keys, n * w)
        say()
        say("## %s keys, %s: read probe %.0f GB/s (one read of the keys: %.3f ms)" % (
            name, {"u": "uniform random bits", "n": "standard normal", "e": "all equal"}[dist], rate, n * w / rate / 1e6))
        for descending in ORDERS:
            a_ms, _ = timed(lambda: p.argsort(d, keys, n, descending=descending, keysOut=full_k, indexOut=full_i))
            want_i = full_i.toHost()[:max(KS)].copy()
            want_k = full_k.toHost()[:max(KS)].view(udt).copy()
            say("%s %-10s argsort + keys out %8.3f ms" % (name, "descending" if descending else "ascending", a_ms))
            d.setParam("topk.algo", 1)
            for k in KS:
                s_ms, ts = timed(lambda: p.topk(d, keys, n, k, descending=descending, keysOut=out_k, indexOut=out_i))
                ok = np.array_equal(out_i.toHost()[:k], want_i[:k]) and np.array_equal(out_k.toHost()[:k].view(udt), want_k[:k])
                say("    k = %8d  select %8.3f ms  argsort / select %6.2f  keys read at %.2f of the probe's rate  [%s]  %s" % (
                    k, s_ms, a_ms / s_ms, (n * w / s_ms / 1e6) / rate, " ".join("%.3f" % t for t in ts), "OK" if ok else "MISMATCH"))
            d.setParam("topk.algo", -1)
    for b in (keys, full_k, full_i, out_k, out_i):
        b.release()

p.close()
DeviceUtils.deallocate(d)
