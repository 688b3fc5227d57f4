#!/usr/bin/env python3
"""Times of adlhip_sort_rows_typed next to what else sorts the rows of the same matrix.

    python tools/sort_rows_bench.py [--reps 5] [--quick] [--out profiles/sort_rows_bench.txt]

Six shapes of 64 Mi keys each, from 2 Mi rows of 32 keys to 2 rows of 32 Mi; int32, float32 and int64 keys; sorted keys with the
columns ("keys+idx") and sorted keys alone ("keys").  Per case, device time (events on torch's stream around the call, median of
`reps` runs after one warm-up; every run takes the next of a few input tensors that together exceed the 256 MiB cache) of
  sort_rows   adlhip_sort_rows_typed as "sort.rows_algo" = -1 runs it: the row kernel up to 4096 columns, the flat path above
  other path  the same call on the flat path where the default is the row kernel ("sort.rows_algo" = 0)
  torch       torch.sort(t, dim=-1, stable=True) on the same tensor (it always returns int64 indices)
  copy        adlhip_probe_copy of half the bytes the call must move -- the keys read, the keys and the columns written --, the floor
  flat sort   the same N keys as ONE array: adlhip_argsort_typed with its sorted keys (keys+idx), adlhip_sort_keys_typed in place on a
              copy made outside the timed window (keys) -- what the rows cost on top of a sort that ignores them
  before      what the library offered for the job before this entry point: adlhip_topk_rows_typed with k == cols where cols <= 2048;
              a host loop of adlhip_argsort_typed, one call per row, where rows <= 64; nothing ("-") in between
The default path's result is compared with torch's (values, and columns where asked) and with the other path's before it is counted.
--quick: int32 only, 2 timed runs, no torch.
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


def timed(run, prep=None):
    times = []
    for r in range(reps + 1):
        if prep:
            prep(r)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(r)
        e1.record()
        torch.cuda.synchronize()
        if r:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def work_for(nbytes):
    p._scratch(d, 0, nbytes)
    return p.m_work.ptr(), p.m_work.getSize()


def size_of(fn, *a):
    wb = ctypes.c_size_t()
    check(fn(d._h, *a, ctypes.byref(wb)), fn.__name__)
    return wb.value


def measure(dtype, rows, cols, want_index):
    n, kb, kt = rows * cols, torch.empty(0, dtype=dtype).element_size(), KEY_TYPE[dtype]
    g = torch.Generator(device="cuda").manual_seed(2026)
    copies = max(2, -(-2 * CACHE_BYTES // (n * kb)))   # together at least twice the cache
    if dtype.is_floating_point:
        ins = [torch.randn((rows, cols), dtype=dtype, device="cuda", generator=g) for _ in range(copies)]
    else:
        ins = [torch.randint(-(1 << 30), 1 << 30, (rows, cols), dtype=dtype, device="cuda", generator=g) for _ in range(copies)]
    vals = torch.empty((rows, cols), dtype=dtype, device="cuda")
    idx = torch.empty((rows, cols), dtype=torch.int32, device="cuda") if want_index else None
    iptr = idx.data_ptr() if want_index else None
    out = {}

    def sort_rows(algo):
        d.setParam("sort.rows_algo", algo)
        try:
            w, wb = work_for(size_of(lib.adlhip_sort_rows_scratch_bytes, kt, rows, cols))
            return timed(lambda r: check(lib.adlhip_sort_rows_typed(d._h, kt, 0, ins[r % copies].data_ptr(), rows, cols, cols, vals.data_ptr(),
                                                                    iptr, w, wb), "sort_rows"))
        finally:
            d.setParam("sort.rows_algo", -1)

    out["sort_rows"] = sort_rows(-1)
    last = ins[reps % copies]   # the input of the last timed run
    mine = (vals.clone(), idx.clone() if want_index else None)
    ok = True
    if not args.quick:
        ref = torch.sort(last, dim=-1, stable=True)
        ok = torch.equal(mine[0], ref.values) and (not want_index or torch.equal(mine[1].to(torch.int64) & 0xffffffff, ref.indices))
        del ref
        out["torch"] = timed(lambda r: torch.sort(ins[r % copies], dim=-1, stable=True))
    if cols <= 4096:
        out["other"] = sort_rows(0)
        ok = ok and torch.equal(mine[0], vals) and (not want_index or torch.equal(mine[1], idx))
    del mine

    half = (n * kb + n * kb + (4 * n if want_index else 0)) // 2 // 16 * 16
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    out["copy"] = timed(lambda r: check(lib.adlhip_probe_copy(d._h, dst.data_ptr(), src.data_ptr(), half), "probe_copy"))
    del src, dst

    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    if want_index:
        check(lib.adlhip_sort_typed_scratch_bytes(d._h, kt, 2, 0, n, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "scratch")
        w, wb = work_for(c.value)
        out["flat"] = timed(lambda r: check(lib.adlhip_argsort_typed(d._h, kt, 0, ins[r % copies].data_ptr(), vals.data_ptr(), iptr, w, wb, n),
                                            "argsort"))
    else:
        check(lib.adlhip_sort_typed_scratch_bytes(d._h, kt, 0, 0, n, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "scratch")
        w, wb = work_for(c.value)
        tmp = torch.empty(a.value, dtype=torch.uint8, device="cuda")
        out["flat"] = timed(lambda r: check(lib.adlhip_sort_keys_typed(d._h, kt, 0, vals.data_ptr(), tmp.data_ptr(), w, wb, n), "sort_keys"),
                            prep=lambda r: vals.copy_(ins[r % copies]))
        del tmp

    if cols <= 2048:
        w, wb = work_for(size_of(lib.adlhip_topk_rows_scratch_bytes, kt, rows, cols, cols))
        out["before"] = timed(lambda r: check(lib.adlhip_topk_rows_typed(d._h, kt, 0, ins[r % copies].data_ptr(), rows, cols, cols, cols,
                                                                         vals.data_ptr(), iptr, w, wb), "topk_rows"))
        out["before_what"] = "topk_rows k=cols"
    elif rows <= 64:
        check(lib.adlhip_sort_typed_scratch_bytes(d._h, kt, 2, 0, cols, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "scratch")
        w, wb = work_for(c.value)
        loop_idx = idx if want_index else torch.empty((rows, cols), dtype=torch.int32, device="cuda")   # (the argsort always writes it)

        def loop(r):
            base = ins[r % copies].data_ptr()
            for row in range(rows):
                check(lib.adlhip_argsort_typed(d._h, kt, 0, base + row * cols * kb, vals.data_ptr() + row * cols * kb,
                                               loop_idx.data_ptr() + row * cols * 4, w, wb, cols), "argsort")

        out["before"] = timed(loop)
        out["before_what"] = "argsort per row"
    del ins, vals, idx
    torch.cuda.empty_cache()
    return out, ok


def ms(v):
    return "%9.3f" % v if v is not None else "%9s" % "-"


N = 1 << args.shift
SHAPES = [(N >> 5, 32), (N >> 10, 1 << 10), (N >> 12, 1 << 12), (N >> 16, 1 << 16), (N >> 20, 1 << 20), (2, N >> 1)]
SHAPES = [s for s in dict.fromkeys(SHAPES) if s[0] >= 1]   # (a rehearsal with a small --shift folds or drops the long rows)
say("# sort_rows_bench: %d keys per shape, ascending; median of %d timed runs per case after one warm-up, rotating inputs; device %s"
    % (N, reps, d.getDeviceName()))
say("# sort_rows: the default path (row kernel up to 4096 columns, flat above); other: the flat path where the default is the row kernel")
say()
say("%-8s %8s %9s %-8s %9s %9s %9s %9s %9s %9s  %-17s %s" % ("keys", "rows", "cols", "output", "sort_rows", "other", "torch", "copy", "flat sort",
                                                          "before", "(before is)", "sort_rows / copy, / flat sort"))
for dtype in ((torch.int32,) if args.quick else (torch.int32, torch.float32, torch.int64)):
    for rows, cols in SHAPES:
        for want_index in (True, False):
            m, ok = measure(dtype, rows, cols, want_index)
            say("%-8s %8d %9d %-8s %s %s %s %s %s %s  %-17s %6.1f %6.2f  %s" % (
                str(dtype).replace("torch.", ""), rows, cols, "keys+idx" if want_index else "keys", ms(m["sort_rows"]), ms(m.get("other")),
                ms(m.get("torch")), ms(m["copy"]), ms(m["flat"]), ms(m.get("before")), m.get("before_what", "-"),
                m["sort_rows"] / m["copy"], m["sort_rows"] / m["flat"], "OK" if ok else "MISMATCH"))

sorter.close()
