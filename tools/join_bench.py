#!/usr/bin/env python3
"""Times of adlhip_join_sorted_typed and adlhip_expand_runs next to the intersection of the same inputs, a copy of the bytes their
models count, what a caller composes without them, and torch on the same tensors.

    python tools/join_bench.py [--reps 7] [--inner 3] [--scale 1] [--join-only] [--out profiles/join_bench_64m.txt]

Shapes: 32 Mi + 32 Mi elements and 64 Mi + 64 Ki; --scale divides both (rehearsals).  Keys int32 and int64.  Key patterns:
  duplicate-free keys, of B's elements none, half or all in A (A's keys are distinct even numbers, the part of B that is not shared
  distinct odd ones); keys drawn from 2^20 values, B cut to 4 Mi elements so that T is about 4 na; one key with 2^16 x 2^10 rows (among distinct others).
The join is the inner join with both index outputs, at cap = T (the counting call has been made; its time is reported on its own).
Each next to
  intersection         adlhip_set_op_typed INTERSECTION with the index output: on duplicate-free inputs the same rows' positions
                       in A (the parent's function; duplicate-free patterns only)
  copy probe           adlhip_probe_copy of as many bytes as the model says the call moves (half of them read, half written)
  torch composition    what a caller composes without it: two torch.searchsorted, a subtraction, torch.cumsum,
                       torch.repeat_interleave (which syncs with the host) and index arithmetic
and, for the expansion (int32 and 8-byte values, the counts of the 2^20-values pattern), torch.repeat_interleave and the copy probe.
The bytes-moved model of the join: (na + nb) x key bytes + 8 T -- A and B read once, the rows written once; of the expansion:
num_runs x (4 + value bytes) + T x value bytes.

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round (the slow contender: a third as many samples of one call), and the median counts.  Everything runs on
torch's stream and is timed with torch.cuda events; every buffer is allocated before the timed runs, and every result is compared with
the torch composition's before it is reported; a mismatch is marked in the table and makes the exit status 1.
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
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--scale", type=int, default=1)
ap.add_argument("--join-only", action="store_true")
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
NP = {torch.int32: np.int32, torch.int64: np.int64}
SHAPES = [((32 << 20) // args.scale, (32 << 20) // args.scale), ((64 << 20) // args.scale, (64 << 10) // args.scale)]
say("# join_bench: per contender the median of %d samples of %d calls each, taken in turns after one warm-up round; device %s%s"
    % (reps, inner, d.getDeviceName(), "; the join and the expansion alone" if args.join_only else ""))


def sample(run, calls):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = run()
        del out
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def in_turns(contenders):
    """contenders: [(label, run, slow)] -> {label: (median, samples)}"""
    times = {label: [] for label, _, _ in contenders}
    for r in range(reps + 1):
        for label, run, slow in contenders:
            if slow and r > max(2, reps // 3):
                continue
            t = sample(run, 1 if slow else inner)
            if r:
                times[label].append(t)
    return {label: (statistics.median(ts), ts) for label, ts in times.items()}


def distinct(n, g, odd):
    """n distinct numbers in rising order, even or odd: the running sum of random steps"""
    steps = torch.randint(1, 8, (n,), dtype=torch.int64, device="cuda", generator=g)
    return torch.cumsum(steps, 0) * 2 + (1 if odd else 0)


def inputs(pattern, dtype, na, nb, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if pattern.startswith("unique"):
        shared = {"unique, 0 % of B in A": 0.0, "unique, 50 % of B in A": 0.5, "unique, 100 % of B in A": 1.0}[pattern]
        a = distinct(na, g, False)
        ns = int(min(nb, na) * shared) if shared < 1.0 else min(nb, na)
        part = a[torch.arange(ns, device="cuda") * (na // max(ns, 1))] if ns else a[:0]
        b = torch.sort(torch.cat((part, distinct(nb - ns, g, True)))).values
    elif pattern == "2^20 values":
        a = torch.sort(torch.randint(0, 1 << 20, (na,), dtype=torch.int64, device="cuda", generator=g)).values
        nb = min(nb, (4 << 20) // args.scale)   # every value about 4 times in B: T is about 4 na
        b = torch.sort(torch.randint(0, 1 << 20, (nb,), dtype=torch.int64, device="cuda", generator=g)).values
    else:   # one key 2^16 times in A and 2^10 times in B, among distinct keys that do not meet
        ra, rb = min(1 << 16, na // 2), min(1 << 10, nb // 2)
        a = torch.sort(torch.cat((distinct(na - ra, g, False), torch.full((ra,), 1001, dtype=torch.int64, device="cuda")))).values
        b = torch.sort(torch.cat((distinct(nb - rb, g, True) + 2000, torch.full((rb,), 1001, dtype=torch.int64, device="cuda")))).values
    return a.to(dtype), b.to(dtype)


def torch_join(a, b):
    lo = torch.searchsorted(b, a)
    m = torch.searchsorted(b, a, right=True) - lo
    start = torch.cumsum(m, 0) - m
    ia = torch.repeat_interleave(torch.arange(a.numel(), device=a.device), m)
    return ia, lo[ia] + (torch.arange(ia.numel(), device=a.device) - start[ia])


nmax = max(a + b for a, b in SHAPES)
probe_src = torch.empty(nmax * 24, dtype=torch.uint8, device="cuda")
probe_dst = torch.empty(nmax * 24, dtype=torch.uint8, device="cuda")
summary, mismatches = [], []


def probe(nbytes):
    half = min((nbytes // 2 + 15) // 16 * 16, probe_src.numel())
    return lambda: check(lib.adlhip_probe_copy(d._h, probe_dst.data_ptr(), probe_src.data_ptr(), half), "probe_copy")


def report(title, contenders, res, n, model, first):
    for label, _, _ in contenders:
        ms, ts = res[label]
        say("    %-28s %8.3f ms  %6.2f Gelem/s  %6.0f GB/s of the model  (min %.3f, max %.3f)" % (label, ms, n / ms / 1e6, model / ms / 1e6, min(ts), max(ts)))
    t = res[first][0]
    ratios = ["%s / %s = %.3f" % (first, label, t / res[label][0]) for label, _, _ in contenders[1:]]
    if ratios:
        say("    " + ";  ".join(ratios))
    summary.append((title, t, [(label, t / res[label][0]) for label, _, _ in contenders[1:]]))


def join_case(pattern, dtype, a, b):
    na, nb = a.numel(), b.numel()
    kdt, kb = NP[dtype], a.element_size()
    cnt = torch.empty(1, dtype=torch.int64, device="cuda")
    p.joinSorted(d, "inner", W(a, kdt), W(b, kdt), na, nb, countOut=W(cnt, np.uint64))
    total = int(cnt.item())
    cap = max(total, 1)   # (no rows: the filling call still runs, with room for one)
    ia, ib = torch.empty(cap, dtype=torch.int32, device="cuda"), torch.empty(cap, dtype=torch.int32, device="cuda")
    kout, xout, scnt = torch.empty(na, dtype=dtype, device="cuda"), torch.empty(na, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")

    def count():
        p.joinSorted(d, "inner", W(a, kdt), W(b, kdt), na, nb, countOut=W(cnt, np.uint64))

    def join():
        p.joinSorted(d, "inner", W(a, kdt), W(b, kdt), na, nb, cap=cap, indexA=W(ia, np.uint32), indexB=W(ib, np.uint32), countOut=W(cnt, np.uint64))

    def intersection():
        p.setOp(d, "intersection", W(a, kdt), W(b, kdt), W(kout, kdt), na, nb, indexOut=W(xout, np.uint32), countOut=W(scnt, np.uint32))

    join()
    wa, wb = torch_join(a, b)
    ok = total == wa.numel() and torch.equal(ia[:total].to(torch.int64) & 0xffffffff, wa) and torch.equal(ib[:total].to(torch.int64) & 0xffffffff, wb)
    del wa, wb
    model = (na + nb) * kb + 8 * total
    contenders = [("join", join, False), ("join, counting call", count, False)]
    if not args.join_only:
        if pattern.startswith("unique"):
            contenders.append(("intersection + index", intersection, False))
        contenders += [("copy probe (model bytes)", probe(model), False), ("torch composition", lambda: torch_join(a, b), True)]
    res = in_turns(contenders)
    title = "%s, %s, %d + %d" % (pattern, str(dtype).replace("torch.", ""), na, nb)
    mismatches.extend([] if ok else [title])
    say()
    say("## join: %s elements, T = %d (%s)" % (title, total, "OK" if ok else "MISMATCH with the torch composition"))
    report("join " + title, contenders, res, na + nb, model, "join")
    torch.cuda.empty_cache()


def expand_case(vdtype, counts):
    n = counts.numel()
    vals = torch.randint(0, 1 << 30, (n,), dtype=torch.int64, device="cuda").to(vdtype)
    want = torch.repeat_interleave(vals, counts.to(torch.int64))
    total, vb = want.numel(), vals.element_size()
    got = s.repeat_interleave(vals, counts, output_size=total)
    ok = torch.equal(got, want)
    del got, want
    reps64 = counts.to(torch.int64)
    model = n * (4 + vb) + total * vb
    contenders = [("expansion", lambda: s.repeat_interleave(vals, counts, output_size=total), False)]
    if not args.join_only:
        contenders += [("copy probe (model bytes)", probe(model), False),
                       ("torch.repeat_interleave", lambda: torch.repeat_interleave(vals, reps64, output_size=total), False)]
    res = in_turns(contenders)
    title = "%s values, %d runs" % (str(vdtype).replace("torch.", ""), n)
    mismatches.extend([] if ok else [title])
    say()
    say("## expansion: %s, T = %d (%s)" % (title, total, "OK" if ok else "MISMATCH with torch.repeat_interleave"))
    report("expansion " + title, contenders, res, n + total, model, "expansion")
    torch.cuda.empty_cache()


PATTERNS = ("unique, 0 % of B in A", "unique, 50 % of B in A", "unique, 100 % of B in A", "2^20 values", "one key 2^16 x 2^10")
for na, nb in SHAPES:
    for dtype in (torch.int32, torch.int64):
        for i, pattern in enumerate(PATTERNS):
            if pattern == "2^20 values" and nb < na:
                continue   # (64 Mi + 64 Ki from 2^20 values: T = 4 Mi, nothing the other patterns do not show)
            a, b = inputs(pattern, dtype, na, nb, 1 + i)
            join_case(pattern, dtype, a, b)
            del a, b
g = torch.Generator(device="cuda").manual_seed(9)
na = (32 << 20) // args.scale
keys = torch.sort(torch.randint(0, 1 << 20, (na,), dtype=torch.int32, device="cuda", generator=g)).values
counts = torch.unique_consecutive(keys, return_counts=True)[1].to(torch.int32)     # 2^20 runs of about 32 rows
for vdtype in (torch.int32, torch.int64):
    expand_case(vdtype, counts)
del keys

say()
say("## summary: ms, and the ratio to every other contender")
for title, t, ratios in summary:
    say("    %-70s %8.3f ms  %s" % (title, t, "  ".join("x %s %.3f" % r for r in ratios)))
s.close()
if mismatches:
    say("MISMATCH in %d cases: %s" % (len(mismatches), mismatches))
    sys.exit(1)
