#!/usr/bin/env python3
"""Times of adlhip_histogram_range_typed and adlhip_bincount_typed next to the calls they are compared with, and next to torch on the
same tensors.

    python tools/histogram_bench.py [n = 64 Mi] [--reps 9] [--inner 4] [--out profiles/histogram_bench_64m.txt]

LDS path: int32 and float32 keys into 256 and 4096 range bins, int32 bincount into 256 bins and into the LDS limit, each on uniform
keys, on all-equal keys and on standard-normal float32 (for the integer cases scaled to the bins and rounded), each next to
  read probe           adlhip_probe_read of the keys' bytes: the model is one read of the keys
  torch                torch.histc (range) / torch.bincount on the same tensor
Sorted path: int32 bincount into 128 Ki and 1 Mi bins (uniform token ids), next to adlhip_sort_keys_typed of a copy of the keys alone,
adlhip_unique_typed with counts, and torch.bincount.

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round, and the median counts.  Library calls are timed with hipEvents on the handle's stream, torch with
torch.cuda events; every buffer is allocated before the timed runs.  Before a case is timed the library's counts are compared with
numpy's: the range mode with searchsorted on the keys' and edges' order-preserving codes (the order of the contract: -0 below +0,
where numpy.histogram holds them equal), bincount with numpy.bincount.  A case that differs is marked MISMATCH, left out of the
summary, and makes the tool exit with status 1."""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=4)
ap.add_argument("--out", default=None)
ap.add_argument("--note", default=None, help="a line for the head of the file")
args = ap.parse_args()
n, reps, inner = args.n, args.reps, args.inner
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
limit = d.getParam("debug.histogram_lds_bins")
say("# histogram_bench: n = %d (%.0f Mi) keys; per contender the median of %d samples of %d calls each, taken in turns after one "
    "warm-up round; LDS limit %d bins; device %s" % (n, n / (1 << 20), reps, inner, limit, d.getDeviceName()))
if args.note:
    say("# " + args.note)


def sample_lib(run):
    DeviceUtils.waitForCompletion(d)
    sw = Stopwatch(d)
    sw.start()
    for _ in range(inner):
        run()
    sw.stop()
    DeviceUtils.waitForCompletion(d)
    return sw.getMs() / inner


def sample_torch(run):
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
    """contenders: [(label, sampler, run)] -> {label: (median, samples)}"""
    times = {label: [] for label, _, _ in contenders}
    for r in range(reps + 1):
        for label, sampler, run in contenders:
            t = sampler(run)
            if r:
                times[label].append(t)
    return {label: (statistics.median(ts), ts) for label, ts in times.items()}


keys32 = Buffer(d, n, np.uint32)            # int32 or float32 keys, as bits
sink = Buffer(d, 16, np.uint8)
counts = Buffer(d, 1 << 20, np.uint32)
rng = np.random.default_rng(8)
normal = rng.standard_normal(n, dtype=np.float32)
uniform = rng.random(n, dtype=np.float32)
summary = []
mismatches = []


def codes(a):
    """the ascending order-preserving code of int32 / float32 values (typed_kernels.hpp: key_enc)"""
    b = a.view(np.uint32)
    if a.dtype == np.int32:
        return b ^ np.uint32(0x80000000)
    return b ^ np.where(b >> np.uint32(31) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def range_counts(keys, edges):
    """the contract's counts with the last bin closed (histogram_oracle.py): bin = (edges <= key on codes) - 1"""
    kc, ec = codes(keys), codes(edges)
    bins = edges.size - 1
    b = np.searchsorted(ec, kc, side="right").astype(np.int64) - 1
    want = np.bincount(b[(b >= 0) & (b < bins)], minlength=bins)
    below = np.flatnonzero(ec[:bins] < ec[bins])
    want[below[-1] if below.size else bins - 1] += np.count_nonzero(kc == ec[bins])
    return want


def report(title, res, order, extra):
    for label in order:
        ms, ts = res[label]
        say("    %-34s %8.3f ms  %6.2f Gkeys/s  (min %.3f, max %.3f)" % (label, ms, n / ms / 1e6, min(ts), max(ts)))
    say("    " + extra)


# ---- LDS path -------------------------------------------------------------------------------------------------
def lds_case(title, host_keys, dtype, bins, edges_host):
    """edges_host: the range mode's edges (dtype), or None for bincount"""
    keys32.write(host_keys.view(np.uint32))
    DeviceUtils.waitForCompletion(d)
    kb = Buffer(dtype=dtype)
    kb.setRawPtr(d, keys32.m_ptr, n)
    cb = Buffer(dtype=np.uint32)
    cb.setRawPtr(d, counts.m_ptr, bins)
    t_keys = torch.from_numpy(host_keys).cuda()
    if edges_host is not None:
        eb = Buffer(d, bins + 1, dtype)
        eb.write(edges_host)
        DeviceUtils.waitForCompletion(d)
        run = lambda: p.histogramRange(d, kb, n, eb, bins, include_upper=True, countsOut=cb)   # noqa: E731
        want = range_counts(host_keys, edges_host)
        lo, hi = float(edges_host[0]), float(edges_host[-1])
        t_in = t_keys if t_keys.dtype == torch.float32 else t_keys.to(torch.float32)   # (torch.histc takes floats only)
        tname, trun = "torch.histc", lambda: torch.histc(t_in, bins=bins, min=lo, max=hi)
    else:
        eb = None
        run = lambda: p.binCount(d, kb, n, bins, countsOut=cb)   # noqa: E731
        want = np.bincount(host_keys[(host_keys >= 0) & (host_keys < bins)], minlength=bins)
        tname, trun = "torch.bincount", lambda: torch.bincount(t_keys, minlength=bins)
    say()
    say("## " + title)
    run()   # sizes the scratch outside the timed runs
    ok = np.array_equal(cb.toHost().astype(np.int64), want)
    probe = lambda: check(lib.adlhip_probe_read(d._h, keys32.ptr(), 4 * n, sink.ptr()), "probe_read")   # noqa: E731
    res = in_turns([("histogram", sample_lib, run), ("read probe (the keys' bytes)", sample_lib, probe), (tname, sample_torch, trun)])
    h, r, t = res["histogram"][0], res["read probe (the keys' bytes)"][0], res[tname][0]
    report(title, res, ("histogram", "read probe (the keys' bytes)", tname),
           "result %s;  histogram / read probe = %.2f (model 1.0);  histogram / %s = %.2f" % ("OK" if ok else "MISMATCH", h / r, tname, h / t))
    if ok:
        summary.append((title, h, "%.2f x one read; %.2f x %s" % (h / r, h / t, tname)))
    else:
        mismatches.append(title)
    if eb is not None:
        eb.release()
    del t_keys
    torch.cuda.empty_cache()


for bins in (256, 4096):
    iedges = np.linspace(0, 1 << 20, bins + 1).astype(np.int32)
    fedges = np.linspace(0.0, 1.0, bins + 1).astype(np.float32)
    dists_i = (("uniform", (uniform * np.float32(1 << 20)).astype(np.int32)), ("all equal", np.full(n, 12345, np.int32)),
               ("normal", np.clip((normal * np.float32(1 << 17)).astype(np.int32) + (1 << 19), 0, (1 << 20) - 1).astype(np.int32)))
    for dname, k in dists_i:
        lds_case("range, int32 keys, %d bins, %s" % (bins, dname), k, np.int32, bins, iedges)
    del dists_i
    nedges = np.linspace(-4.0, 4.0, bins + 1).astype(np.float32)
    for dname, k, e in (("uniform", uniform, fedges), ("all equal", np.full(n, 0.3, np.float32), fedges), ("normal", normal, nedges)):
        lds_case("range, float32 keys, %d bins, %s" % (bins, dname), k, np.float32, bins, e)
for bins in (256, limit):
    dists = (("uniform", (uniform * np.float32(bins)).astype(np.int32)), ("all equal", np.full(n, bins // 3, np.int32)),
             ("normal", np.clip((normal * np.float32(bins / 8)).astype(np.int32) + bins // 2, 0, bins - 1).astype(np.int32)))
    for dname, k in dists:
        lds_case("bincount, int32 keys, %d bins, %s" % (bins, dname), k, np.int32, bins, None)
    del dists

# ---- sorted path ----------------------------------------------------------------------------------------------
work = Buffer(d, 0, np.uint8)
tmp = Buffer(d, n, np.uint32)
scopy = Buffer(d, n, np.uint32)
uniq, ucounts, ucount = Buffer(d, n, np.int32), Buffer(d, n, np.uint32), Buffer(d, 1, np.uint32)
for bins in (128 << 10, 1 << 20):
    host = (uniform * np.float32(bins)).astype(np.int32)
    np.minimum(host, bins - 1, out=host)
    keys32.write(host.view(np.uint32))
    DeviceUtils.waitForCompletion(d)
    kb = Buffer(dtype=np.int32)
    kb.setRawPtr(d, keys32.m_ptr, n)
    cb = Buffer(dtype=np.uint32)
    cb.setRawPtr(d, counts.m_ptr, bins)
    t_keys = torch.from_numpy(host).cuda()
    tk, tv, wb, ub = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.adlhip_sort_typed_scratch_bytes(d._h, 1, 0, 0, n, ctypes.byref(tk), ctypes.byref(tv), ctypes.byref(wb)), "scratch")
    check(lib.adlhip_unique_scratch_bytes(d._h, 1, n, 0, ctypes.byref(ub)), "scratch")
    if work.getSize() < max(wb.value, ub.value):
        work.setSize(max(wb.value, ub.value))

    def sort_alone():   # what the sorted path pays before its boundary launches: the copy and the keys sort
        p.copy(d, scopy, keys32, n)
        check(lib.adlhip_sort_keys_typed(d._h, 1, 0, scopy.ptr(), tmp.ptr(), work.ptr(), work.getSize(), n), "sort_keys_typed")

    def unique_counts():
        check(lib.adlhip_unique_typed(d._h, 1, 0, keys32.ptr(), n, uniq.ptr(), ucounts.ptr(), None, None, None, ucount.ptr(), work.ptr(),
                                      work.getSize()), "unique_typed")

    title = "bincount, int32 keys, %d bins (sorted path), uniform" % bins
    say()
    say("## " + title)
    run = lambda: p.binCount(d, kb, n, bins, countsOut=cb)   # noqa: E731
    run()
    ok = np.array_equal(cb.toHost().astype(np.int64), np.bincount(host, minlength=bins))
    res = in_turns([("bincount", sample_lib, run), ("copy + sort_keys_typed", sample_lib, sort_alone), ("unique_typed with counts", sample_lib, unique_counts),
                    ("torch.bincount", sample_torch, lambda: torch.bincount(t_keys, minlength=bins))])
    h, s, u, t = (res[k][0] for k in ("bincount", "copy + sort_keys_typed", "unique_typed with counts", "torch.bincount"))
    report(title, res, ("bincount", "copy + sort_keys_typed", "unique_typed with counts", "torch.bincount"),
           "result %s;  bincount / (copy + sort) = %.2f;  bincount / unique with counts = %.2f;  bincount / torch.bincount = %.2f"
           % ("OK" if ok else "MISMATCH", h / s, h / u, h / t))
    if ok:
        summary.append((title, h, "%.2f x copy + sort; %.2f x unique with counts; %.2f x torch.bincount" % (h / s, h / u, h / t)))
    else:
        mismatches.append(title)
    del t_keys
    torch.cuda.empty_cache()

say()
say("## summary: ms")
for title, ms, text in summary:
    say("    %-58s %7.3f ms  (%s)" % (title, ms, text))
if mismatches:
    say()
    say("## MISMATCH in %d case(s), left out of the summary: %s" % (len(mismatches), "; ".join(mismatches)))

p.close()
for b in (keys32, sink, counts, work, tmp, scopy, uniq, ucounts, ucount):
    b.release()
DeviceUtils.deallocate(d)
sys.exit(1 if mismatches else 0)
