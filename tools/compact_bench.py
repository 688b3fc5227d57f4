#!/usr/bin/env python3
"""Times of adlhip_compact_flagged and adlhip_compact_if_typed next to the calls they are compared with, and next to torch on the same
tensors.

    python tools/compact_bench.py [n = 64 Mi] [--reps 9] [--inner 4] [--out profiles/compact_bench_64m.txt]

Cases, each at 1 %, 50 % and 99 % selected: flagged int32 items, flagged int64 items, flagged positions only (nonzero), compact_if on
float32 keys without and with a 4-byte value, and the flagged stable partition of int32 items.  Each next to
  copy probe           adlhip_probe_copy of as many bytes as the model says the call moves (half of them read, half written)
  run-length encode    adlhip_run_length_encode on n all-distinct 4-byte keys with offsets (once per run of the tool): the nearest
                       existing kernel -- the same three launches, keys read twice, n keys and n offsets written
  torch                torch.masked_select / torch.nonzero / t[t < x] on the same tensors
The bytes-moved model: the count launch reads the predicate's input (n flag bytes, or n keys); the emit launch reads it again, plus the
items or values, and writes S elements per output (a partition: n).

One sample is `inner` calls back to back between two events, divided by `inner`; the contenders of a case take turns, `reps` samples
each after one warm-up round, and the median counts.  Library calls are timed with hipEvents on the handle's stream, torch with
torch.cuda events; every buffer is allocated before the timed runs, and the library's result is compared with torch's before it is
counted.
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--inner", type=int, default=4)
ap.add_argument("--out", default=None)
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
say("# compact_bench: n = %d (%.0f Mi) elements; per contender the median of %d samples of %d calls each, taken in turns after one "
    "warm-up round; device %s" % (n, n / (1 << 20), reps, inner, d.getDeviceName()))


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


# buffers shared by every case: two 8-byte arrays for the copy probe, the flags, items / keys / values of both widths, the outputs
big_a, big_b = Buffer(d, 2 * n, np.uint64), Buffer(d, 2 * n, np.uint64)
flags = Buffer(d, n, np.uint8)
i32, i64, f32 = Buffer(d, n, np.int32), Buffer(d, n, np.int64), Buffer(d, n, np.float32)
o32, o64, of32, idx, count = Buffer(d, n, np.int32), Buffer(d, n, np.int64), Buffer(d, n, np.float32), Buffer(d, n, np.uint32), Buffer(d, 1, np.uint32)
rng = np.random.default_rng(8)
host_i32 = rng.integers(-1 << 31, 1 << 31, size=n, dtype=np.int64).astype(np.int32)
host_i64 = rng.integers(-1 << 62, 1 << 62, size=n, dtype=np.int64)
host_f32 = rng.random(n, dtype=np.float32)          # uniform in [0, 1): t < x selects the fraction x
u = rng.random(n, dtype=np.float32)
i32.write(host_i32)
i64.write(host_i64)
f32.write(host_f32)
DeviceUtils.waitForCompletion(d)
t_i32, t_i64, t_f32 = torch.from_numpy(host_i32).cuda(), torch.from_numpy(host_i64).cuda(), torch.from_numpy(host_f32).cuda()

# the nearest existing kernel, once
rle_keys = Buffer(d, n, np.uint32)
rle_keys.write(np.arange(n, dtype=np.uint32))
DeviceUtils.waitForCompletion(d)
r = p.runLengthEncode(d, rle_keys, n, offsets=True)
rle = in_turns([("run-length encode", sample_lib,
                 lambda: p.runLengthEncode(d, rle_keys, n, offsets=r.offsets, uniqueOut=r.unique, countOut=r.count))])["run-length encode"][0]
say()
say("## run-length encode, %d all-distinct 4-byte keys, with offsets: %.3f ms (model: %d bytes, %.0f GB/s)" % (n, rle, 16 * n, 16 * n / rle / 1e6))
for b in (rle_keys, r.unique, r.offsets, r.count):
    b.release()


def probe(nbytes):
    half = (nbytes // 2 + 15) // 16 * 16
    return lambda: check(lib.adlhip_probe_copy(d._h, big_b.ptr(), big_a.ptr(), half), "probe_copy")


summary = []
for frac in (0.01, 0.5, 0.99):
    host_flags = (u < frac).astype(np.uint8)
    flags.write(host_flags)
    DeviceUtils.waitForCompletion(d)
    t_mask = torch.from_numpy(host_flags).cuda().to(torch.bool)
    S = int(host_flags.sum())
    Sf = int((host_f32 < np.float32(frac)).sum())
    th = np.float32(frac)
    cases = [
        ("flagged int32 items", 2 * n + 4 * n + 4 * S,
         lambda: p.compactFlagged(d, flags, n, items=i32, itemsOut=o32, countOut=count),
         ("torch.masked_select", lambda: torch.masked_select(t_i32, t_mask)),
         lambda: np.array_equal(o32.toHost(S), torch.masked_select(t_i32, t_mask).cpu().numpy())),
        ("flagged int64 items", 2 * n + 8 * n + 8 * S,
         lambda: p.compactFlagged(d, flags, n, items=i64, itemsOut=o64, countOut=count),
         ("torch.masked_select", lambda: torch.masked_select(t_i64, t_mask)),
         lambda: np.array_equal(o64.toHost(S), torch.masked_select(t_i64, t_mask).cpu().numpy())),
        ("flagged, positions only", 2 * n + 4 * S,
         lambda: p.compactFlagged(d, flags, n, indexOut=idx, countOut=count),
         ("torch.nonzero", lambda: torch.nonzero(t_mask)),
         lambda: np.array_equal(idx.toHost(S).astype(np.int64), torch.nonzero(t_mask).flatten().cpu().numpy())),
        ("compact_if float32 keys", 2 * 4 * n + 4 * Sf,
         lambda: p.compactIf(d, f32, n, "lt", th, keysOut=of32, countOut=count),
         ("t[t < x]", lambda: t_f32[t_f32 < float(th)]),
         lambda: np.array_equal(of32.toHost(Sf), t_f32[t_f32 < float(th)].cpu().numpy())),
        ("compact_if float32 keys + int32 values", 2 * 4 * n + 4 * n + 8 * Sf,
         lambda: p.compactIf(d, f32, n, "lt", th, values=i32, keysOut=of32, valuesOut=o32, countOut=count),
         ("t[m], v[m]", lambda: (lambda m: (t_f32[m], t_i32[m]))(t_f32 < float(th))),
         lambda: np.array_equal(o32.toHost(Sf), t_i32[t_f32 < float(th)].cpu().numpy())),
        ("flagged partition, int32 items", 2 * n + 4 * n + 4 * n,
         lambda: p.compactFlagged(d, flags, n, items=i32, partition=True, itemsOut=o32, countOut=count),
         ("torch.cat([t[m], t[~m]])", lambda: torch.cat([t_i32[t_mask], t_i32[~t_mask]])),
         lambda: np.array_equal(o32.toHost(), torch.cat([t_i32[t_mask], t_i32[~t_mask]]).cpu().numpy())),
    ]
    for title, model, run, (tname, trun), verify in cases:
        say()
        say("## %s, %.0f %% selected" % (title, 100 * frac))
        run()   # sizes the scratch outside the timed runs
        ok = verify()
        res = in_turns([("compact", sample_lib, run), ("copy probe (model bytes)", sample_lib, probe(model)), (tname, sample_torch, trun)])
        for label in ("compact", "copy probe (model bytes)", tname):
            ms, ts = res[label]
            say("    %-28s %8.3f ms  %6.2f Gelem/s  %6.0f GB/s of the model  (min %.3f, max %.3f)" % (
                label, ms, n / ms / 1e6, model / ms / 1e6, min(ts), max(ts)))
        c, cp, t = res["compact"][0], res["copy probe (model bytes)"][0], res[tname][0]
        say("    result %s;  model %d bytes;  compact / copy probe = %.2f (model 1.0);  compact / %s = %.2f;  compact / run-length encode = %.2f"
            % ("OK" if ok else "MISMATCH", model, c / cp, tname, c / t, c / rle))
        summary.append((title, frac, c, cp, t, tname))
        torch.cuda.empty_cache()
    del t_mask

say()
say("## summary: ms (x the copy probe of the model's bytes; x torch)")
for title, frac, c, cp, t, tname in summary:
    say("    %-40s %3.0f %%  %7.3f ms  (%.2f x model; %.2f x %s)" % (title, 100 * frac, c, c / cp, c / t, tname))

p.close()
for b in (big_a, big_b, flags, i32, i64, f32, o32, o64, of32, idx, count):
    b.release()
DeviceUtils.deallocate(d)
