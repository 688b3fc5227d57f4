#!/usr/bin/env python3
"""Times of adlhip_search_sorted_typed next to the bytes it must move, the histogram's search, torch and the merge.

    python tools/search_bench.py [--reps 7] [--inner 2] [--scale 1] [--out profiles/search_bench_64m.txt]

64 Mi needles (--scale divides them and the largest sequence: rehearsals), uniform random and sorted, searched in sorted sequences of
256, 4096, 64 Ki, 1 Mi and 64 Mi keys drawn from the same distribution.  Keys int32, float32 and int64; both sides.  Each next to
  copy probe           adlhip_probe_copy of the bytes the call must move: n needles read, n positions written (half of them read, half
                       written).  The sequence's bytes are not in it: what is read of it depends on the needles
  histogram            adlhip_histogram_range_typed of the needles with the sequence as edges, for the sequences of 256 and 4096 keys
                       (255 and 4095 bins): the same search in LDS with an atomic add in place of a store
  torch                torch.searchsorted on the same tensors (torch.bucketize is the same kernel with the arguments swapped; it is
                       timed once per dtype)
  merge                for sorted needles, adlhip_merge_typed of the sequence and the needles with the index output alone: the positions of
                       both inputs in the merged order, from which either bound follows

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round, and the median counts.  Everything runs on torch's stream and is timed with torch.cuda events; every
buffer is allocated before the timed runs, and the search's result is compared with torch's before it is counted.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch  # before the HIP back-end is loaded: one HIP runtime per process

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import TorchSorter, _lib  # noqa: E402
from oclradixsort_amd._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=2)
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
reps, inner = args.reps, args.inner
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    if args.out:   # kept current: a run that is cut short leaves what it measured
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


s = TorchSorter(0)
d, p, lib = s.device, s.pprims, _lib.load()
W = s._wrap
NP = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}
N = (64 << 20) // args.scale
LENGTHS = [256, 4096, 64 << 10, 1 << 20, (64 << 20) // args.scale]
say("# search_bench: per contender the median of %d samples of %d calls each, taken in turns after one warm-up round; device %s; table "
    "in LDS: %d codes" % (reps, inner, d.getDeviceName(), d.getParam("debug.search_lds_keys")))


def sample(run):
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
    """contenders: [(label, run)] -> {label: (median, samples)}"""
    times = {label: [] for label, _ in contenders}
    for r in range(reps + 1):
        for label, run in contenders:
            t = sample(run)
            if r:
                times[label].append(t)
    return {label: (statistics.median(ts), ts) for label, ts in times.items()}


def keys_of(dtype, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.float32:
        return torch.rand(n, device="cuda", generator=g) - 0.5
    if dtype == torch.int32:
        return torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    return torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)


probe_src = torch.empty(N * 6, dtype=torch.uint8, device="cuda")     # half of the largest model: 8 + 4 bytes per needle
probe_dst = torch.empty(N * 6, dtype=torch.uint8, device="cuda")
pos = torch.empty(N, dtype=torch.int32, device="cuda")
summary = []
for dtype in (torch.int32, torch.float32, torch.int64):
    kdt, kb = NP[dtype], torch.empty(0, dtype=dtype).element_size()
    dname = str(dtype).replace("torch.", "")
    uniform = keys_of(dtype, N, 1)
    needle_sets = [("uniform", uniform), ("sorted", torch.sort(uniform).values)]
    model = N * (kb + 4)
    half = (model // 2 + 15) // 16 * 16
    for m in LENGTHS:
        seq = torch.sort(keys_of(dtype, m, 2)).values
        counts = hwork = None
        if m in (256, 4096):
            counts = p.histogramRange(d, W(uniform, kdt), N, W(seq, kdt), m - 1)   # (sizes the work buffer outside the timed runs)
        midx = torch.empty(N + m, dtype=torch.int32, device="cuda")
        for nname, needles in needle_sets:
            say()
            say("## %s keys, %s needles, %d needles in %d sorted keys" % (dname, nname, N, m))
            ok = True
            for right in (False, True):
                p.searchSorted(d, W(seq, kdt), W(needles, kdt), W(pos, np.uint32), m, N, right=right)
                ok &= torch.equal(pos.to(torch.int64), torch.searchsorted(seq, needles, right=right))
            contenders = [
                ("search left", lambda: p.searchSorted(d, W(seq, kdt), W(needles, kdt), W(pos, np.uint32), m, N)),
                ("search right", lambda: p.searchSorted(d, W(seq, kdt), W(needles, kdt), W(pos, np.uint32), m, N, right=True)),
                ("copy probe (needles + positions)", lambda: check(lib.adlhip_probe_copy(d._h, probe_dst.data_ptr(), probe_src.data_ptr(), half),
                                                                   "probe_copy")),
                ("torch.searchsorted left", lambda: torch.searchsorted(seq, needles)),
                ("torch.searchsorted right", lambda: torch.searchsorted(seq, needles, right=True)),
            ]
            if m == LENGTHS[0] and nname == "uniform":
                contenders.append(("torch.bucketize right", lambda: torch.bucketize(needles, seq, right=True)))
            if counts is not None:
                contenders.append(("histogram, %d edges" % m, lambda: p.histogramRange(d, W(needles, kdt), N, W(seq, kdt), m - 1, countsOut=counts)))
            if nname == "sorted":
                contenders.append(("merge, index output", lambda: p.mergeKeys(d, W(seq, kdt), W(needles, kdt), None, m, N, indexOut=W(midx, np.uint32))))
            for _, run in contenders[-2:]:
                run()   # (sizes the scratch outside the timed runs)
            res = in_turns(contenders)
            for label, _ in contenders:
                ms, ts = res[label]
                say("    %-34s %8.3f ms  %6.2f Gneedles/s  %6.0f GB/s of the model  (min %.3f, max %.3f)" % (
                    label, ms, N / ms / 1e6, model / ms / 1e6, min(ts), max(ts)))
            L, R, cp = res["search left"][0], res["search right"][0], res["copy probe (needles + positions)"][0]
            tl, tr = res["torch.searchsorted left"][0], res["torch.searchsorted right"][0]
            hist = res["histogram, %d edges" % m][0] if counts is not None else None
            mrg = res["merge, index output"][0] if nname == "sorted" else None
            say("    result %s;  model %d bytes;  search / copy probe = %.2f / %.2f;  search / torch = %.2f / %.2f%s%s" % (
                "OK" if ok else "MISMATCH", model, L / cp, R / cp, L / tl, R / tr,
                ";  search right / histogram = %.2f" % (R / hist) if hist else "", ";  search right / merge = %.2f" % (R / mrg) if mrg else ""))
            summary.append((dname, nname, m, L, R, cp, tl, tr, hist, mrg))
        if counts is not None:
            counts.release()
        del seq, midx
        torch.cuda.empty_cache()
    del uniform, needle_sets
    torch.cuda.empty_cache()

say()
say("## summary: ms left / right (x the copy probe; x torch.searchsorted; the histogram at the same edges; the merge with the index output)")
for dname, nname, m, L, R, cp, tl, tr, hist, mrg in summary:
    say("    %-8s %-8s needles in %9d keys  %7.3f / %7.3f ms  (%.2f / %.2f x copy %.3f ms; %.2f / %.2f x torch %.3f / %.3f ms%s%s)" % (
        dname, nname, m, L, R, L / cp, R / cp, cp, L / tl, R / tr, tl, tr,
        "; histogram %.3f ms" % hist if hist else "", "; merge %.3f ms" % mrg if mrg else ""))
s.close()
