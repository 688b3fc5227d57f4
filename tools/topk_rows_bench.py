#!/usr/bin/env python3
"""Times of adlhip_topk_rows_typed: its row kernel next to its per-row loop, torch.topk and one read of the keys.

    python tools/topk_rows_bench.py [--reps 5] [--quick] [--out profiles/topk_rows_bench.txt]

Per shape (rows, cols, k), f32 keys, descending: device time (events around the call on torch's stream, median of `reps` runs after one
warm-up) of
  kernel  adlhip_topk_rows_typed with "topk.rows_algo" = 1: one workgroup per row, everything in LDS
  loop    the same call with "topk.rows_algo" = 0: `rows` runs of the 1-D top-k ("topk.algo" at its default), same build, same session
  torch   torch.topk(t, k, dim=-1, largest=True, sorted=True) on the same tensor
  read    adlhip_probe_read_ex over the rows * cols keys (the better of plain and non-temporal loads): the floor is one read
and the ratio of each path to the read.  Keys are uniform in [0, 1) at every shape and standard normal at two of them.  The kernel's
result is compared with the loop's (columns and key bits) before it is counted.
A second table times kernel and loop alone for 256 rows and for 32 rows at doubling cols: "L" is the largest measured cols at which
the kernel is not slower than the loop in both series -- what "topk.rows_algo" = -1 should use as its limit on cols.
--quick: the first table's shapes only, without the loop at more than 4096 rows.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import Buffer, DeviceUtils, Stopwatch, TorchSorter, _lib  # noqa: E402
from oclradixsort_amd._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps = args.reps
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    if args.out:   # kept current: a run that is cut short leaves what it measured
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


sorter = TorchSorter(0)
d, p = sorter.device, sorter.pprims
lib = _lib.load()
say("# topk_rows_bench: f32 keys, descending; median of %d timed runs per case after one warm-up; device %s" % (reps, d.getDeviceName()))


def wrap(t, dtype):
    b = Buffer(dtype=dtype)
    b.setRawPtr(d, t.data_ptr(), t.numel())
    return b


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
    return statistics.median(times)


def timed_torch(run):
    times = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def read_ms(t):
    nbytes = t.numel() * t.element_size()
    sink = Buffer(d, 16, np.uint8)
    best = min(timed(lambda: check(lib.adlhip_probe_read_ex(d._h, t.data_ptr(), nbytes, sink.ptr(), hints, 8), "probe_read_ex"))
               for hints in (0, 1))
    sink.release()
    return best


def keys_of(rows, cols, dist):
    g = torch.Generator(device="cuda").manual_seed(2026)
    if dist == "uniform":
        return torch.rand((rows, cols), dtype=torch.float32, device="cuda", generator=g)
    return torch.randn((rows, cols), dtype=torch.float32, device="cuda", generator=g)


def measure(rows, cols, k, dist, with_torch=True, with_loop=True):
    t = keys_of(rows, cols, dist)
    keys = wrap(t, np.float32)
    out = {}
    res = {}
    for name, algo in (("kernel", 1), ("loop", 0)):
        if name == "loop" and not with_loop:
            continue
        vals = torch.empty((rows, k), dtype=torch.float32, device="cuda")
        idx = torch.empty((rows, k), dtype=torch.int32, device="cuda")
        kb, ib = wrap(vals, np.float32), wrap(idx, np.uint32)
        d.setParam("topk.rows_algo", algo)
        out[name] = timed(lambda: p.topkRows(d, keys, rows, cols, k, descending=True, keysOut=kb, indexOut=ib))
        d.setParam("topk.rows_algo", -1)
        res[name] = (vals.view(torch.int32).clone(), idx.clone())
    ok = "loop" not in res or (torch.equal(res["kernel"][0], res["loop"][0]) and torch.equal(res["kernel"][1], res["loop"][1]))
    if with_torch:
        out["torch"] = timed_torch(lambda: torch.topk(t, k, dim=-1, largest=True, sorted=True))
        out["read"] = read_ms(t)
    del t
    torch.cuda.empty_cache()
    return out, ok


SHAPES = [(16384, 128, 8, "uniform"), (4096, 32768, 64, "uniform"), (256, 131072, 50, "uniform"), (256, 131072, 50, "normal"),
          (256, 262144, 50, "uniform"), (32, 1 << 20, 100, "uniform"), (32, 1 << 20, 100, "normal"), (8, 4 << 20, 100, "uniform")]
say()
say("%7s %9s %5s %-8s %10s %10s %10s %10s   %s" % ("rows", "cols", "k", "keys", "kernel ms", "loop ms", "torch ms", "read ms",
                                                   "kernel / loop / torch over read"))
for rows, cols, k, dist in SHAPES:
    with_loop = not (args.quick and rows > 4096)
    m, ok = measure(rows, cols, k, dist, with_loop=with_loop)
    loop = m.get("loop")
    say("%7d %9d %5d %-8s %10.3f %10s %10.3f %10.3f   %7.1f %7s %7.1f  %s" % (
        rows, cols, k, dist, m["kernel"], "%.3f" % loop if loop is not None else "-", m["torch"], m["read"], m["kernel"] / m["read"],
        "%.1f" % (loop / m["read"]) if loop is not None else "-", m["torch"] / m["read"], "OK" if ok else "MISMATCH"))

if not args.quick:
    say()
    say("# kernel against loop at doubling cols, k = 50, uniform keys")
    say("%7s %9s %10s %10s   %s" % ("rows", "cols", "kernel ms", "loop ms", "kernel / loop"))
    wins = {}
    for rows in (256, 32):
        for sh in range(14, 23):
            cols = 1 << sh
            if rows * cols > (1 << 28):
                continue
            m, ok = measure(rows, cols, 50, "uniform", with_torch=False)
            say("%7d %9d %10.3f %10.3f   %6.2f  %s" % (rows, cols, m["kernel"], m["loop"], m["kernel"] / m["loop"], "OK" if ok else "MISMATCH"))
            if m["kernel"] <= m["loop"]:
                wins.setdefault(cols, set()).add(rows)
    both = [c for c, r in wins.items() if r == {256, 32}]
    say()
    say("L (largest measured cols at which the kernel is not slower than the loop in both series): %s" % (max(both) if both else "none"))

sorter.close()
