#!/usr/bin/env python3
"""Times of the typed sorts (signed, float and descending keys, argsort, typed pairs) next to the unsigned sort and the copy probe.

    python tools/typed_sort_bench.py [n = 64 Mi] [--reps 5] [--out profiles/typed_sort_bench_64m.txt]

Per case: device time (hipEvents around the call) of `reps` runs on the same input after one warm-up, their median in ms and in
Gkeys/s, and the per-kernel times of one more run with "profile" on.  Keys are uniform random bits (generated on the device) unless
the case says "normal" (standard-normal floats, generated on the host).  The (f32, u32) pairs are sorted twice: by the index path of
adlhip_sort_pairs_typed and by adlhip_key_encode + adlhip_radix_sort_soa32 + adlhip_key_decode.  The codec kernels are set beside
adlhip_probe_copy on the same byte count.  Every result is checked for order (neighbouring keys, on the host) before it is counted.
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
ap.add_argument("--out", default=None)
args = ap.parse_args()
n, reps = args.n, args.reps
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


def ordinal(bits, kind):
    """int64 ordinal of 4-byte keys: the value (u, i) or the sign-magnitude reading of the bits (f)"""
    if kind == "u":
        return bits.astype(np.int64)
    s = bits.view(np.int32).astype(np.int64)
    return s if kind == "i" else np.where(s >= 0, s, -(s & 0x7fffffff) - 1)


def in_order(bits, kind, descending):
    o = ordinal(bits, kind)
    return bool(np.all(o[:-1] >= o[1:]) if descending else np.all(o[:-1] <= o[1:]))


d = DeviceUtils.allocate()
p = Pprims()
lib = _lib.load()
say("# typed_sort_bench: n = %d (%.0f Mi) keys, %d timed runs per case after one warm-up; device %s" % (n, n / (1 << 20), reps, d.getDeviceName()))

pristine = Buffer(d, n, np.uint32)
pristine.generate(n, seed=2026)            # uniform random bits
normal = Buffer(d, n, np.float32)
normal.write(np.random.default_rng(7).standard_normal(n).astype(np.float32))
DeviceUtils.waitForCompletion(d)


def timed(label, setup, run, verify, keys_per_run=n):
    """setup() restores the input (untimed), run() enqueues the call"""
    times = []
    for r in range(reps + 1):
        setup()
        DeviceUtils.waitForCompletion(d)
        sw = Stopwatch(d)
        sw.start()
        run()
        sw.stop()
        DeviceUtils.waitForCompletion(d)
        if r:
            times.append(sw.getMs())
    ok = verify()
    d.toggleProfiling(True)
    d.profile(reset=True)
    setup()
    run()
    DeviceUtils.waitForCompletion(d)
    prof = d.profile(reset=True)
    d.toggleProfiling(False)
    med = statistics.median(times)
    say("%-44s median %8.3f ms  %7.2f Gkeys/s  [%s]  %s" % (label, med, keys_per_run / med / 1e6, " ".join("%.3f" % t for t in times),
                                                             "OK" if ok else "OUT OF ORDER"))
    say("    kernels: " + "  ".join("%s=%.3f" % (k, ms / c) + ("x%d" % c if c > 1 else "") for k, (c, ms) in prof.items()))
    return med, prof


def keys_case(label, dtype, kind, source, descending, typed=True):
    b = Buffer(d, n, dtype)
    try:
        return timed(label, lambda: b.write(source, n),
                     (lambda: p.sortKeys(d, b, n, descending=descending)) if typed else (lambda: p.radixSort(d, b, n)),
                     lambda: in_order(b.toHost().view(np.uint32), kind, descending))
    finally:
        b.release()


say()
say("## keys only (encode in place, unsigned sort, decode in place)")
base, _ = keys_case("u32 ascending, adlhip_radix_sort_u32", np.uint32, "u", pristine, False, typed=False)
keys_case("u32 ascending, adlhip_sort_keys_typed", np.uint32, "u", pristine, False)
keys_case("u32 descending", np.uint32, "u", pristine, True)
keys_case("i32 ascending", np.int32, "i", pristine, False)
f32_med, f32_prof = keys_case("f32 ascending, uniform random bits", np.float32, "f", pristine, False)
keys_case("f32 descending, uniform random bits", np.float32, "f", pristine, True)
runs0 = d.getParam("stat.net_runs")
keys_case("f32 ascending, standard normal", np.float32, "f", normal, False)
say("    the large sort's safety net ran %d times in these %d sorts (\"stat.net_runs\")" % (d.getParam("stat.net_runs") - runs0, reps + 2))

say()
say("## codec kernels beside the copy probe (%d MiB read + %d MiB written each)" % (n * 4 >> 20, n * 4 >> 20))
a = Buffer(d, n, np.uint32)
b = Buffer(d, n, np.uint32)
a.write(pristine, n)


def codec_rate(label, call):
    """per-launch time of `call` from "profile": reps launches after one warm-up, nothing else in the table"""
    d.toggleProfiling(True)
    call()
    DeviceUtils.waitForCompletion(d)
    d.profile(reset=True)
    for _ in range(reps):
        call()
    DeviceUtils.waitForCompletion(d)
    prof = d.profile(reset=True)
    d.toggleProfiling(False)
    (name, (c, ms)), = prof.items()
    return label, name, c, ms / c


rows = [
    codec_rate("probe_copy b <- a", lambda: check(lib.adlhip_probe_copy(d._h, b.ptr(), a.ptr(), 4 * n), "probe_copy")),
    codec_rate("key_encode f32 b <- a (out of place)", lambda: check(lib.adlhip_key_encode(d._h, 2, 0, b.ptr(), a.ptr(), n), "key_encode")),
    codec_rate("key_decode f32 b <- a (out of place)", lambda: check(lib.adlhip_key_decode(d._h, 2, 0, b.ptr(), a.ptr(), n), "key_decode")),
    codec_rate("key_encode f32 a <- a (in place, as the sort runs it)", lambda: check(lib.adlhip_key_encode(d._h, 2, 0, a.ptr(), a.ptr(), n), "key_encode")),
    codec_rate("key_decode f32 a <- a (in place)", lambda: check(lib.adlhip_key_decode(d._h, 2, 0, a.ptr(), a.ptr(), n), "key_decode")),
]
copy_ms = rows[0][3]
for label, name, c, per in rows:
    say("%-56s %7.3f ms per launch (%d launches)  %7.1f GB/s moved  %.2f of the copy probe's rate" % (
        label, per, c, 2 * 4 * n / per / 1e6, copy_ms / per))
same = np.array_equal(a.toHost(), pristine.toHost())
say("    in-place encode and decode ran %d times each, in turn: a == the input again: %s" % (reps + 1, "OK" if same else "MISMATCH"))
a.release()
b.release()

say()
say("## argsort and pairs (index path: no codec sweep)")
kb = Buffer(d, n, np.float32)
ko = Buffer(d, n, np.float32)
io = Buffer(d, n, np.uint32)
kb.write(pristine, n)
timed("f32 argsort + sorted keys", lambda: None, lambda: p.argsort(d, kb, n, keysOut=ko, indexOut=io),
      lambda: in_order(ko.toHost().view(np.uint32), "f", False))


def indices_ok():
    idx = io.toHost()
    seen = np.zeros(n, dtype=bool)
    seen[idx] = True
    return bool(seen.all()) and in_order(pristine.toHost()[idx], "f", False)


timed("f32 argsort, indices only", lambda: None, lambda: p.argsort(d, kb, n, indexOut=io), indices_ok)
ko.release()
io.release()

vb = Buffer(d, n, np.uint32)
iota = Buffer(d, n, np.uint32)
iota.write(np.arange(n, dtype=np.uint32))
DeviceUtils.waitForCompletion(d)


def restore_pairs():
    kb.write(pristine, n)
    vb.write(iota, n)


def pairs_ok():
    keys = kb.toHost().view(np.uint32)
    vals = vb.toHost()
    src = pristine.toHost()
    o = ordinal(keys, "f")
    stable = np.all((o[:-1] < o[1:]) | ((o[:-1] == o[1:]) & (vals[:-1] < vals[1:])))
    return bool(stable) and np.array_equal(src[vals], keys)


timed("(f32, u32) pairs, index path", restore_pairs, lambda: p.sortPairs(d, kb, vb, n), pairs_ok)

tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
check(lib.adlhip_radix_sort_scratch_bytes(d._h, 3, n, ctypes.byref(tb), ctypes.byref(wb)), "scratch")
p._scratch(d, 2 * tb.value, wb.value)


def soa_path():
    check(lib.adlhip_key_encode(d._h, 2, 0, kb.ptr(), kb.ptr(), n), "key_encode")
    check(lib.adlhip_radix_sort_soa32(d._h, kb.ptr(), vb.ptr(), p.m_tmp.ptr(), ctypes.c_void_p(p.m_tmp.m_ptr + tb.value), p.m_work.ptr(),
                                      p.m_work.getSize(), n, 32), "soa32")
    check(lib.adlhip_key_decode(d._h, 2, 0, kb.ptr(), kb.ptr(), n), "key_decode")


timed("(f32, u32) pairs, encode + soa32 + decode", restore_pairs, soa_path, pairs_ok)

for x in (kb, vb, iota, pristine, normal):
    x.release()
p.close()
DeviceUtils.deallocate(d)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
