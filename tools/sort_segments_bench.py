#!/usr/bin/env python3
"""Times of adlhip_sort_segments_typed next to what else sorts the segments of the same array.

    python tools/sort_segments_bench.py [--reps 5] [--quick] [--out profiles/sort_segments_bench.txt]

Six shapes of 64 Mi keys each; int32, float32 and int64 keys; sorted keys with the positions inside the segment.
  equal 32 / equal 1024   every segment of that length (what adlhip_sort_rows_typed sorts too)
  uniform 1..64 / 1..4096 lengths drawn uniformly
  heavy tail              lengths floor(u^(-1 / 1.2)) for uniform u, truncated at 4096: most segments of one to three keys, a few long
  heavy tail + 32 Mi      one segment of 32 Mi keys in front of the same: max_segment is 32 Mi, which forces the flat path
Per case, device time (events on torch's stream around the call; median of `reps` rounds after one warm-up round; in every round the
contenders take turns, and every round takes the next of a few input tensors that together exceed the 256 MiB cache) of
  segments    adlhip_sort_segments_typed with max_segment = the longest segment, "sort.segments_algo" = -1: the segment kernel (plan,
              one sort launch) while that is <= 4096, the flat path above
  flat        the same call under "sort.segments_algo" = 0
  sort_rows   adlhip_sort_rows_typed on the equal shapes
  torch       two stable torch.sort calls -- by key, then the segment ids in that order -- and the two gathers that apply them
  copy        adlhip_probe_copy of half the bytes the call must move -- the keys read, the keys and the indices written --, the floor
The default path's result is compared with the flat path's (bit for bit) and with torch's values before it is counted.
--quick: int32 only, 2 timed rounds, no torch.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oclradixsort_amd import TorchSorter, _lib  # noqa: E402
from oclradixsort_amd._lib import check  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quick", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--shift", type=int, default=26, help="log2 of the keys per shape (26: the 64 Mi of the table; smaller to rehearse)")
args = ap.parse_args()
reps = 2 if args.quick else args.reps
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
KEY_TYPE = {torch.int32: 1, torch.float32: 2, torch.int64: 4}
CACHE_BYTES = 256 << 20
CAP = 4096


def take_turns(contenders):
    """{name: median ms}: reps + 1 rounds, every contender once per round in the same order, the first round dropped"""
    times = {name: [] for name in contenders}
    for r in range(reps + 1):
        for name, run in contenders.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(r)
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1))
    return {name: statistics.median(t) for name, t in times.items()}


def work_for(nbytes):
    p._scratch(d, 0, nbytes)
    return p.m_work.ptr(), p.m_work.getSize()


def size_of(fn, *a):
    wb = ctypes.c_size_t()
    check(fn(d._h, *a, ctypes.byref(wb)), fn.__name__)
    return wb.value


def offsets_from(lens, n):
    """offsets of the leading segments of `lens` that fill n keys exactly (the last one cut short)"""
    cs = torch.cumsum(lens.to(torch.int64), 0)
    assert int(cs[-1]) >= n, "too few lengths drawn"
    S = int(torch.searchsorted(cs, torch.tensor([n], device=cs.device, dtype=torch.int64))[0]) + 1
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=cs.device), cs[:S - 1], torch.tensor([n], dtype=torch.int64, device=cs.device)])


def heavy_tail(count, g):
    u = torch.rand(count, device="cuda", generator=g, dtype=torch.float64).clamp_min(1e-12)
    return u.pow(-1.0 / 1.2).floor().clamp(1, CAP).to(torch.int64)


def make_offsets(shape, n):
    g = torch.Generator(device="cuda").manual_seed(7)
    if shape.startswith("equal"):
        length = int(shape.split()[1])
        return torch.arange(0, n + 1, length, dtype=torch.int64, device="cuda")
    if shape.startswith("uniform"):
        hi = int(shape.split("..")[1])
        return offsets_from(torch.randint(1, hi + 1, (2 * n // (hi + 1) + 4096,), device="cuda", generator=g), n)
    if shape == "heavy tail":
        return offsets_from(heavy_tail(n // 2 + 4096, g), n)
    tail = offsets_from(heavy_tail(n // 4 + 4096, g), n // 2)   # heavy tail + half of the keys in one segment
    return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), tail + n // 2])


def measure(dtype, shape, n):
    kb, kt = torch.empty(0, dtype=dtype).element_size(), KEY_TYPE[dtype]
    off64 = make_offsets(shape, n)
    S = off64.numel() - 1
    lens = off64[1:] - off64[:-1]
    longest = int(lens.max())
    off32 = off64.to(torch.int32)
    g = torch.Generator(device="cuda").manual_seed(2026)
    copies = max(2, -(-2 * CACHE_BYTES // (n * kb)))   # together at least twice the cache
    if dtype.is_floating_point:
        ins = [torch.randn(n, dtype=dtype, device="cuda", generator=g) for _ in range(copies)]
    else:
        ins = [torch.randint(-(1 << 30), 1 << 30, (n,), dtype=dtype, device="cuda", generator=g) for _ in range(copies)]
    vals = torch.empty(n, dtype=dtype, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    vals2, idx2 = torch.empty_like(vals), torch.empty_like(idx)

    def segments(algo, vout, iout):
        def run(r):
            d.setParam("sort.segments_algo", algo)
            try:
                w, wb = work_for(size_of(lib.adlhip_sort_segments_scratch_bytes, kt, n, S, longest))
                check(lib.adlhip_sort_segments_typed(d._h, kt, 0, ins[r % copies].data_ptr(), n, off32.data_ptr(), S, longest, 0, vout.data_ptr(),
                                                     iout.data_ptr(), None, w, wb), "sort_segments")
            finally:
                d.setParam("sort.segments_algo", -1)
        return run

    contenders = {"segments": segments(-1, vals, idx)}
    if longest <= CAP:
        contenders["flat"] = segments(0, vals2, idx2)
    if shape.startswith("equal"):
        rows, cols = S, longest

        def rows_run(r):
            w, wb = work_for(size_of(lib.adlhip_sort_rows_scratch_bytes, kt, rows, cols))
            check(lib.adlhip_sort_rows_typed(d._h, kt, 0, ins[r % copies].data_ptr(), rows, cols, cols, vals2.data_ptr(), idx2.data_ptr(), w, wb),
                  "sort_rows")
        contenders["sort_rows"] = rows_run
    if not args.quick:
        seg_ids = torch.repeat_interleave(torch.arange(S, device="cuda", dtype=torch.int32), lens)
        kept = {}

        def torch_run(r):
            by_key = torch.sort(ins[r % copies], stable=True).indices
            by_seg = torch.sort(seg_ids[by_key], stable=True).indices
            order = by_key[by_seg]
            kept["values"], kept["order"] = ins[r % copies][order], order
        contenders["torch"] = torch_run
    half = (n * kb + n * kb + 4 * n) // 2 // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    contenders["copy"] = lambda r: check(lib.adlhip_probe_copy(d._h, dst.data_ptr(), src.data_ptr(), half), "probe_copy")
    out = take_turns(contenders)
    ok = True   # every contender ran last on ins[reps % copies]
    if "flat" in contenders:
        ok = torch.equal(vals, vals2) and torch.equal(idx, idx2)
    elif longest > CAP:   # the default was the flat path: nothing else of the library's to compare with
        pass
    if not args.quick:
        ok = ok and torch.equal(vals, kept["values"])
        starts = torch.repeat_interleave(off64[:-1], lens)
        ok = ok and torch.equal((idx.to(torch.int64) & 0xffffffff) + starts, kept["order"])
    del ins, vals, idx, vals2, idx2, src, dst
    torch.cuda.empty_cache()
    return out, S, longest, ok


def ms(v):
    return "%9.3f" % v if v is not None else "%9s" % "-"


def ratio(a, b):
    return "%6.2f" % (a / b) if a is not None and b is not None else "%6s" % "-"


N = 1 << args.shift
SHAPES = ["equal 32", "equal 1024", "uniform 1..64", "uniform 1..4096", "heavy tail", "heavy tail + %d Mi" % (N >> 21)]
say("# sort_segments_bench: %d keys per shape, ascending, keys + local indices; median of %d timed rounds after one warm-up, the contenders"
    % (N, reps))
say("# taking turns, rotating inputs; device %s" % d.getDeviceName())
say("# segments: the default path (segment kernel while the longest segment <= 4096, flat above); flat: \"sort.segments_algo\" = 0")
say()
say("%-8s %-20s %9s %8s %9s %9s %9s %9s %9s  %s" % ("keys", "shape", "segments", "longest", "segments", "flat", "sort_rows", "torch", "copy",
                                                   "segments / sort_rows, / flat, / copy"))
for dtype in ((torch.int32,) if args.quick else (torch.int32, torch.float32, torch.int64)):
    for shape in SHAPES:
        m, S, longest, ok = measure(dtype, shape, N)
        say("%-8s %-20s %9d %8d %s %s %s %s %s  %s %s %s  %s" % (
            str(dtype).replace("torch.", ""), shape, S, longest, ms(m["segments"]), ms(m.get("flat")), ms(m.get("sort_rows")), ms(m.get("torch")),
            ms(m["copy"]), ratio(m["segments"], m.get("sort_rows")), ratio(m["segments"], m.get("flat")), ratio(m["segments"], m["copy"]),
            "OK" if ok else "MISMATCH"))

sorter.close()
