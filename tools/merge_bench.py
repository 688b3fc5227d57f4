#!/usr/bin/env python3
"""Times of adlhip_merge_typed next to what a caller does without it, and next to torch on the same tensors.

    python tools/merge_bench.py [--reps 9] [--inner 4] [--scale 1] [--out profiles/merge_bench_64m.txt]

Shapes: 32 Mi + 32 Mi elements (two shards) and 64 Mi + 64 Ki (a batch merged into an index); --scale divides both (rehearsals).
Keys int32, float32 and int64; keys only, keys + positions, keys + a float32 value.  Each next to
  copy probe           adlhip_probe_copy of as many bytes as the model says the call moves (half of them read, half written)
  concat + sort        two device copies into one array, then adlhip_sort_keys_typed (keys only), adlhip_argsort_typed (positions) or
                       adlhip_sort_pairs_typed (values): what a caller does today
  torch                torch.sort(torch.cat((a, b))) (positions: its indices; values: gathered through them)
The bytes-moved model of the merge: (na + nb) x (2 x key bytes + 2 x value bytes + 4 if positions) -- every element read once and
written once.  The partition launch's reads (one search per 2048 outputs) are not in it.

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round, and the median counts.  Everything runs on torch's stream and is timed with torch.cuda events; every
buffer is allocated before the timed runs, and the merge's result is compared with torch's before it is counted.
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=4)
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
NP = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32}
SHAPES = [((32 << 20) // args.scale, (32 << 20) // args.scale), ((64 << 20) // args.scale, (64 << 10) // args.scale)]
say("# merge_bench: per contender the median of %d samples of %d calls each, taken in turns after one warm-up round; device %s"
    % (reps, inner, d.getDeviceName()))


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
        t = torch.rand(n, device="cuda", generator=g) - 0.5
    elif dtype == torch.int32:
        t = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    else:
        t = torch.randint(-(1 << 62), 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    return torch.sort(t).values


nmax = max(a + b for a, b in SHAPES)
probe_src = torch.empty(nmax * 12, dtype=torch.uint8, device="cuda")     # half of the largest model: 2 x 8 + 2 x 4 bytes per element
probe_dst = torch.empty(nmax * 12, dtype=torch.uint8, device="cuda")
summary = []
for na, nb in SHAPES:
    n = na + nb
    va, vb = torch.rand(na, device="cuda"), torch.rand(nb, device="cuda")
    vout, vcat = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    for dtype in (torch.int32, torch.float32, torch.int64):
        kdt, kb = NP[dtype], torch.empty(0, dtype=dtype).element_size()
        a, b = keys_of(dtype, na, 1), keys_of(dtype, nb, 2)
        kout, kcat, ksorted = (torch.empty(n, dtype=dtype, device="cuda") for _ in range(3))
        W = s._wrap
        forms = [
            ("keys only", 2 * kb,
             lambda: p.mergeKeys(d, W(a, kdt), W(b, kdt), W(kout, kdt), na, nb),
             lambda: (p.copy(d, W(kcat, kdt), W(a, kdt), na), p.copy(d, W(kcat[na:], kdt), W(b, kdt), nb), p.sortKeys(d, W(kcat, kdt), n)),
             lambda: torch.sort(torch.cat((a, b))).values,
             lambda: torch.equal(kout, torch.sort(torch.cat((a, b))).values)),
            ("keys + positions", 2 * kb + 4,
             lambda: p.mergeKeys(d, W(a, kdt), W(b, kdt), W(kout, kdt), na, nb, indexOut=W(idx, np.uint32)),
             lambda: (p.copy(d, W(kcat, kdt), W(a, kdt), na), p.copy(d, W(kcat[na:], kdt), W(b, kdt), nb),
                      p.argsort(d, W(kcat, kdt), n, keysOut=W(ksorted, kdt), indexOut=W(idx, np.uint32))),
             lambda: torch.sort(torch.cat((a, b)), stable=True),
             lambda: torch.equal(idx.to(torch.int64) & 0xffffffff, torch.sort(torch.cat((a, b)), stable=True).indices)),
            ("keys + float32 value", 2 * kb + 8,
             lambda: p.mergePairs(d, W(a, kdt), W(va, np.float32), W(b, kdt), W(vb, np.float32), W(kout, kdt), W(vout, np.float32), na, nb),
             lambda: (p.copy(d, W(kcat, kdt), W(a, kdt), na), p.copy(d, W(kcat[na:], kdt), W(b, kdt), nb),
                      p.copy(d, W(vcat, np.float32), W(va, np.float32), na), p.copy(d, W(vcat[na:], np.float32), W(vb, np.float32), nb),
                      p.sortPairs(d, W(kcat, kdt), W(vcat, np.float32), n)),
             lambda: (lambda r: (r.values, torch.cat((va, vb))[r.indices]))(torch.sort(torch.cat((a, b)), stable=True)),
             lambda: torch.equal(vout, torch.cat((va, vb))[torch.sort(torch.cat((a, b)), stable=True).indices])),
        ]
        for title, per_elem, merge, resort, trun, verify in forms:
            model = n * per_elem
            half = (model // 2 + 15) // 16 * 16
            say()
            say("## %s keys, %s, %d + %d elements" % (str(dtype).replace("torch.", ""), title, na, nb))
            resort()   # (both size their scratch outside the timed runs)
            merge()
            ok = verify()
            res = in_turns([("merge", merge),
                            ("copy probe (model bytes)", lambda: check(lib.adlhip_probe_copy(d._h, probe_dst.data_ptr(), probe_src.data_ptr(), half),
                                                                       "probe_copy")),
                            ("concat + sort", resort), ("torch.sort(torch.cat)", trun)])
            for label in ("merge", "copy probe (model bytes)", "concat + sort", "torch.sort(torch.cat)"):
                ms, ts = res[label]
                say("    %-28s %8.3f ms  %6.2f Gelem/s  %6.0f GB/s of the model  (min %.3f, max %.3f)" % (
                    label, ms, n / ms / 1e6, model / ms / 1e6, min(ts), max(ts)))
            m, cp, rs, t = (res[k][0] for k in ("merge", "copy probe (model bytes)", "concat + sort", "torch.sort(torch.cat)"))
            say("    result %s;  model %d bytes;  merge / copy probe = %.2f (model 1.0);  merge / concat + sort = %.2f;  merge / torch = %.2f"
                % ("OK" if ok else "MISMATCH", model, m / cp, m / rs, m / t))
            summary.append((str(dtype).replace("torch.", ""), title, na, nb, m, cp, rs, t))
            torch.cuda.empty_cache()
        if dtype == torch.int32 and na == nb:
            # the grid of the tile kernel: the default (8 workgroups per CU) against 4 and 2 per CU, keys only
            cus = int(d.info.compute_units)
            contenders = []
            for per_cu in (8, 4, 2):
                def run(per_cu=per_cu):
                    d.setParam("debug.merge_grid", per_cu * cus)
                    p.mergeKeys(d, W(a, kdt), W(b, kdt), W(kout, kdt), na, nb)
                contenders.append(("%d workgroups per CU" % per_cu, run))
            res = in_turns(contenders)
            d.setParam("debug.merge_grid", 0)
            say()
            say("## the tile kernel's grid, int32 keys only, %d + %d elements" % (na, nb))
            for label, _ in contenders:
                say("    %-28s %8.3f ms  (min %.3f, max %.3f)" % (label, res[label][0], min(res[label][1]), max(res[label][1])))
        del a, b, kout, kcat, ksorted
    del va, vb, vout, vcat, idx

say()
say("## summary: ms (x the copy probe of the model's bytes; x concat + sort; x torch)")
for dt, title, na, nb, m, cp, rs, t in summary:
    say("    %-8s %-22s %9d + %-9d %7.3f ms  (%.2f x model; %.2f x concat + sort %.3f ms; %.2f x torch %.3f ms)" % (
        dt, title, na, nb, m, m / cp, m / rs, rs, m / t, t))
s.close()
