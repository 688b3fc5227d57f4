#!/usr/bin/env python3
"""Times of adlhip_set_op_typed next to the merge of the same inputs, a copy of the bytes its model counts, what a caller composes
without it, and torch on the same tensors.

    python tools/setop_bench.py [--reps 7] [--inner 3] [--scale 1] [--setop-only] [--out profiles/setop_bench_64m.txt]

Shapes: 32 Mi + 32 Mi elements and 64 Mi + 64 Ki; --scale divides both (rehearsals).  Keys int32 and int64, with and without a
float32 value, all four operations, and overlaps of about 0 %, 50 % and 100 %: of B's elements none, half or all occur in A (A's
keys are even numbers drawn at random, the part of B that is not shared odd ones).  One heavily duplicated case: 256 distinct keys.
Each next to
  merge                adlhip_merge_typed of the same inputs (keys, and the value where there is one)
  copy probe           adlhip_probe_copy of as many bytes as the model says the call moves (half of them read, half written)
  merge + unique       the composition available without it: the merge, then adlhip_unique_typed with counts on the merged keys (the
                       caller would still have to compact by the counts); keys only
  torch                torch.cat + torch.unique(return_counts=True) + a mask on the counts (difference: a[~torch.isin(a, b)]); keys only.
                       That is the same operation on inputs without duplicates only: the few keys the random inputs draw twice make
                       its result differ by as many elements (its time is what counts here), and the case of 256 distinct keys
                       leaves it out
The bytes-moved model of a set operation: 2 x (na + nb) x key bytes + S x (key bytes + value bytes) -- the inputs read twice (count
and emit), the result written once.  --setop-only times the set operation alone (the second side of an A/B of two builds).

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round (the two slow contenders: a third as many samples of one call), and the median counts.  Everything runs
on torch's stream and is timed with torch.cuda events; every buffer is allocated before the timed runs, and the count of every
result is compared with the count torch derives from the run lengths of each key before it is reported; a mismatch is marked in
the table and makes the exit status 1.
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
ap.add_argument("--setop-only", action="store_true")
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
OPS = ("intersection", "union", "difference", "symmetric_difference")
SHAPES = [((32 << 20) // args.scale, (32 << 20) // args.scale), ((64 << 20) // args.scale, (64 << 10) // args.scale)]
say("# setop_bench: per contender the median of %d samples of %d calls each, taken in turns after one warm-up round; device %s%s"
    % (reps, inner, d.getDeviceName(), "; the set operation alone" if args.setop_only else ""))


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


def inputs(dtype, na, nb, shared, seed):
    """sorted a (even numbers) and b: `shared` of b's elements are elements of a spread evenly over it, the others odd numbers"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    span = 1 << (30 if dtype == torch.int32 else 61)
    a = torch.sort(torch.randint(-span, span, (na,), dtype=torch.int64, device="cuda", generator=g) * 2).values
    ns = int(nb * shared)
    part = a[(torch.arange(ns, device="cuda") * (na // max(ns, 1)))] if ns else a[:0]
    fresh = torch.randint(-span, span, (nb - ns,), dtype=torch.int64, device="cuda", generator=g) * 2 + 1
    b = torch.sort(torch.cat((part, fresh))).values
    return a.to(dtype), b.to(dtype)


def expected_counts(a, b):
    """the four result sizes from the run lengths m (in a) and n (in b) of every distinct key"""
    u = torch.unique(torch.cat((a, b)))
    m = torch.searchsorted(a, u, right=True) - torch.searchsorted(a, u)
    n = torch.searchsorted(b, u, right=True) - torch.searchsorted(b, u)
    return {"intersection": int(torch.minimum(m, n).sum()), "union": int(torch.maximum(m, n).sum()),
            "difference": int((m - n).clamp(min=0).sum()), "symmetric_difference": int((m - n).abs().sum())}


def torch_equivalent(op, a, b):
    if op == "difference":
        return a[~torch.isin(a, b)]
    u, c = torch.unique(torch.cat((a, b)), return_counts=True)
    return u if op == "union" else u[c == (2 if op == "intersection" else 1)]


nmax = max(a + b for a, b in SHAPES)
probe_src = torch.empty(nmax * 14, dtype=torch.uint8, device="cuda")     # half of the largest model: (2 x 8 + 8 + 4) bytes per element
probe_dst = torch.empty(nmax * 14, dtype=torch.uint8, device="cuda")
summary, mismatches = [], []


def case(title, dtype, a, b, want, valued, ops, with_torch=True):
    na, nb = a.numel(), b.numel()
    n = na + nb
    kdt, kb = NP[dtype], a.element_size()
    va, vb = (torch.rand(na, device="cuda"), torch.rand(nb, device="cuda")) if valued else (None, None)
    kout, merged, uniq = (torch.empty(n, dtype=dtype, device="cuda") for _ in range(3))
    vout = torch.empty(n, device="cuda") if valued else None
    counts = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt, ucnt = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")

    def merge():
        if valued:
            p.mergePairs(d, W(a, kdt), W(va, np.float32), W(b, kdt), W(vb, np.float32), W(merged, kdt), W(vout, np.float32), na, nb)
        else:
            p.mergeKeys(d, W(a, kdt), W(b, kdt), W(merged, kdt), na, nb)

    def compose():
        p.mergeKeys(d, W(a, kdt), W(b, kdt), W(merged, kdt), na, nb)
        p.unique(d, W(merged, kdt), n, counts=W(counts, np.uint32), uniqueOut=W(uniq, kdt), countOut=W(ucnt, np.uint32))

    for op in ops:
        def setop(op=op):
            p.setOp(d, op, W(a, kdt), W(b, kdt), W(kout, kdt), na, nb, valuesA=W(va, np.float32) if valued else None,
                    valuesB=W(vb, np.float32) if valued else None, valuesOut=W(vout, np.float32) if valued else None,
                    countOut=W(cnt, np.uint32))
        setop()
        merge()
        got = int(cnt.item()) & 0xffffffff
        ok = got == want[op] and (got < 2 or bool((kout[1:got] >= kout[:got - 1]).all()))
        model = 2 * n * kb + got * (kb + (4 if valued else 0))
        half = (model // 2 + 15) // 16 * 16
        contenders = [("set operation", setop, False)]
        if not args.setop_only:
            contenders += [("merge", merge, False),
                           ("copy probe (model bytes)",
                            lambda: check(lib.adlhip_probe_copy(d._h, probe_dst.data_ptr(), probe_src.data_ptr(), half), "probe_copy"), False)]
            if not valued:
                compose()
                contenders += [("merge + unique with counts", compose, True)]
                if with_torch:
                    contenders += [("torch", lambda op=op: torch_equivalent(op, a, b), True)]
        res = in_turns(contenders)
        say()
        mismatches.extend([] if ok else [(title, op)])
        say("## %s, %s keys%s, %s, %d + %d elements, S = %d (%s)" % (title, str(dtype).replace("torch.", ""), " + float32 value" if valued else "",
                                                                       op, na, nb, got, "OK" if ok else "MISMATCH: expected %d" % want[op]))
        for label, _, _ in contenders:
            ms, ts = res[label]
            say("    %-28s %8.3f ms  %6.2f Gelem/s  %6.0f GB/s of the model  (min %.3f, max %.3f)" % (
                label, ms, n / ms / 1e6, model / ms / 1e6, min(ts), max(ts)))
        t = res["set operation"][0]
        row = [title, str(dtype).replace("torch.", ""), "+v" if valued else "", op, na, nb, t]
        if not args.setop_only:
            mg, cp = res["merge"][0], res["copy probe (model bytes)"][0]
            text = "    set operation / merge = %.2f;  / copy probe = %.2f (model 1.0)" % (t / mg, t / cp)
            row += [t / mg, t / cp]
            if not valued:
                co = res["merge + unique with counts"][0]
                text += ";  / (merge + unique) = %.3f" % (t / co)
                row += [t / co]
                if with_torch:
                    text += ";  / torch = %.4f" % (t / res["torch"][0])
                    row += [t / res["torch"][0]]
            say(text)
        summary.append(row)
    torch.cuda.empty_cache()


for na, nb in SHAPES:
    for dtype in (torch.int32, torch.int64):
        for shared, name in ((0.0, "overlap 0 %"), (0.5, "overlap 50 %"), (1.0, "overlap 100 %")):
            a, b = inputs(dtype, na, nb, shared, 1 + int(10 * shared))
            want = expected_counts(a, b)
            for valued in (False, True):
                case(name, dtype, a, b, want, valued, OPS)
            del a, b
g = torch.Generator(device="cuda").manual_seed(5)
na = nb = (32 << 20) // args.scale
a = torch.sort(torch.randint(0, 256, (na,), dtype=torch.int32, device="cuda", generator=g)).values
b = torch.sort(torch.randint(0, 256, (nb,), dtype=torch.int32, device="cuda", generator=g)).values
case("256 distinct keys", torch.int32, a, b, expected_counts(a, b), False, OPS, with_torch=False)

say()
say("## summary: ms (x the merge of the same inputs; x the copy probe of the model's bytes; x merge + unique with counts; x torch)")
for row in summary:
    say("    %-18s %-6s%-3s %-21s %9d + %-9d %7.3f ms  %s" % (tuple(row[:7]) + ("  ".join("%.3f" % x for x in row[7:]),)))
if not args.setop_only:
    worst = max((r[7], r) for r in summary if r[0] == "overlap 50 %" and r[3] == "intersection")
    say("    intersection at 50 %% overlap: at most %.2f x the merge of the same inputs (%s)" % (worst[0], "under 2 x" if worst[0] < 2 else "NOT under 2 x"))
s.close()
if mismatches:
    say("MISMATCH in %d cases: %s" % (len(mismatches), mismatches))
    sys.exit(1)
