#!/usr/bin/env python3
"""Soak test of the inter-workgroup look-back protocol: many back-to-back one-sweep sorts of random sizes,
element kinds and key distributions, every result checked (sortedness + multiset checksum on the device
result copied back, full oracle comparison for the smaller ones), fault word checked at every sync.  Every eighth sort
is followed -- while later sorts are already queued -- by the LDS-order self-test on a SECOND handle (the hardware
behaviour "sort.rank" = 1 rests on, adlhip_selftest_lds_order), and one size class reaches past 64 Mi keys (the
pointer-store write-out).  Half of the sorts take the automatic choice (mid-size sort, large sort with its look-back /
cursor passes and the safety net inside its offsets kernel), with "sort.msd2" forced on for some and keys shifted down by a random number of bits.
One kind in ten is a stream compaction between the sorts (a stable partition of the keys by a comparison, values and positions along),
one a histogram (range or bincount, random key type, bins and grid knob, the LDS and the sorted path), one a merge (the keys cut in
two, each part sorted by the library as int32 or float32 keys in either order, then merged with positions and 8-byte values along),
one a set operation (the keys folded onto a random number of distinct values and cut in two, each part sorted by the library, then
a random one of the four operations with positions and 8-byte values along, checked against tests/setop_oracle.py),
one a sorted search (the keys cut into a sequence, sorted by the library as int32 or float32 keys in either order, and needles -- random
ones and elements of the sequence --, either side, random table capacity and grid knob, checked against numpy.searchsorted on the codes),
one a sort within segments (the keys as int32 or float32 in either order, cut into segments of uniform or heavy-tailed lengths with runs
of empty ones, on the segment kernel or the flat path with a random grid knob and index base, checked against one numpy lexsort on
(segment, code)),
one a join (the keys folded and cut in two as for the set operations, a random kind, capacity and "debug.join_grid", checked against
tests/join_oracle.py), one an expansion of runs (counts with stretches of zeros and a few long runs, 8-byte values along).
   python tools/stress.py [--seconds 60]"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle
import ctypes
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import setop_oracle   # the numpy oracle of the set operation tests
import join_oracle    # ... and of the join and expansion tests
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from oclradixsort_amd._lib import check
ap = argparse.ArgumentParser(); ap.add_argument("--seconds", type=float, default=60.0)
ap.add_argument("--skip-before", type=int, default=0, help="replay: draw the first iterations without running them")
ap.add_argument("--stop-after", type=int, default=1 << 30); ap.add_argument("--verbose", action="store_true")
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--mix-rank", action="store_true", help="also draw sort.rank per sort (0 = ballot ranking: the stable large sort's ballot variants)")
args = ap.parse_args()
mix_rng = np.random.RandomState(args.seed + 1)
skip_before, verbose = args.skip_before, args.verbose
d = DeviceUtils.allocate(); p = Pprims()
d2 = DeviceUtils.allocate(); selftests = 0
rng = np.random.RandomState(args.seed)
t_end = time.time() + args.seconds
it = 0; elems = 0; t_mark = time.time()
def checks(a):
    a64 = a.astype(np.uint64)
    return int(a64.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(a64)) if a.size else 0
while time.time() < t_end and it < args.stop_after:
    it += 1
    kind = rng.choice(["u32", "kv", "u64", "soa", "soaw", "compact", "hist", "merge", "setop", "search", "segments", "join", "expand"])
    n = int(2 ** rng.uniform(10, 25.5)) + int(rng.randint(0, 1000))
    if it % 7 == 0: n = int(2 ** rng.uniform(21, 26.3))   # more of the large sort's range
    if kind == "u32" and it % 23 == 0: n = (1 << 26) + int(rng.randint(1, 1 << 22))     # past 256 MiB: pointer stores
    if kind == "u32" and it % 37 == 0: n = int(2 ** rng.uniform(27.1, 28.6))            # 140 Mi ... 400 Mi keys: segments finished by a workgroup each
    algo = int(rng.choice([0, 0, 1, -1, -1, -1])); bits = int(rng.choice([8, 8, 8, 4])); tile = int(rng.choice([-1, -1, 0, 1, 2, 3]))
    if algo < 0: bits, tile = 8, -1   # what the automatic paths run with
    d.setParam("sort.algo", algo); d.setParam("sort.digit_bits", bits); d.setParam("sort.tile", tile)
    if args.mix_rank: d.setParam("sort.rank", int(mix_rng.choice([1, 1, 0])))   # ballot ranking on a third of the sorts (own generator: replays stay aligned)
    d.setParam("sort.msd2", int(rng.choice([1, 1, 1, 2, 3, 4, 5])))   # automatic or a forced form
    dist = rng.choice(["uniform", "lowbits", "fewvals", "sortedish", "shifted", "shifted", "heavy", "vals4096"])
    shift = int(rng.randint(1, 20))
    msd2_mode = d.getParam("sort.msd2")
    if it < skip_before:   # replay: only the draws of the generator (they do not depend on any result)
        if kind == "u32":
            if it % 5 == 0 and n < (1 << 22): rng.choice([16, 20, 24, 28])
            else: rng.randint(1, 4)
        continue
    if verbose: print("it %d %s n=%d algo=%d bits=%d tile=%d msd2=%d dist=%s shift=%d" % (it, kind, n, algo, bits, tile, msd2_mode, dist, shift), flush=True)
    if kind in ("u32", "soa", "kv", "soaw", "compact", "hist", "merge", "setop", "search", "segments", "join", "expand"):
        k = oracle.keys_u32(n, seed=it)
        if dist == "heavy": k = np.where(np.arange(n) % 10 != 0, (k >> np.uint32(8)) | np.uint32(0x37000000), k).astype(np.uint32)
        elif dist == "vals4096": k = (k >> np.uint32(20)) * np.uint32(0x00100801)
        if dist == "lowbits": k &= np.uint32(0xffff)
        elif dist == "fewvals": k = (k % np.uint32(5)) * np.uint32(0x01010101)
        elif dist == "sortedish": k = np.sort(k)
        elif dist == "shifted": k >>= np.uint32(shift)
    if kind == "u32":
        b = Buffer(d, n, np.uint32); b.write(k)
        if it % 5 == 0 and n < (1 << 22):   # a sort on part of the key (stable form of the large sort above 2 Mi keys)
            sb = int(rng.choice([16, 20, 24, 28]))
            p.radixSort(d, b, n, sb)
            out = b.toHost(); b.release()
            assert np.array_equal(out, oracle.sort_u32_bits(k, sb)), (it, kind, n, sb, dist)
            elems += n
            continue
        reps = int(rng.randint(1, 4))
        for _ in range(reps): p.radixSort(d, b, n)          # re-sorting sorted data stresses the low-entropy paths
        if it % 8 == 0:   # the ranking's hardware assumption, checked on another stream while these sorts run
            mism = ctypes.c_uint32(1)
            check(_lib.load().adlhip_selftest_lds_order(d2._h, 256, ctypes.byref(mism)), "selftest")
            assert mism.value == 0, ("lds order self-test", it)
            selftests += 1
        out = b.toHost(); b.release()
        assert np.all(out[1:] >= out[:-1]) and checks(out) == checks(k), (it, kind, n, algo, bits, tile, dist)
        if n < (1 << 22): assert np.array_equal(out, oracle.sort_u32(k)), (it, kind, n)
    elif kind == "kv":
        pr = k.astype(np.uint64) | (np.arange(n, dtype=np.uint64) << np.uint64(32))
        b = Buffer(d, n, np.uint64); b.write(pr); p.radixSort(d, b, n); out = b.toHost(); b.release()
        kk = out & np.uint64(0xffffffff); vv = out >> np.uint64(32)
        assert np.all(kk[1:] >= kk[:-1]); same = kk[1:] == kk[:-1]
        assert np.all(vv[1:][same] > vv[:-1][same]) and checks(out) == checks(pr), (it, kind, n, algo, bits, tile, dist)
    elif kind == "soa":
        v = np.arange(n, dtype=np.uint32)
        kb = Buffer(d, n, np.uint32); vb = Buffer(d, n, np.uint32); kb.write(k); vb.write(v)
        p.radixSortSoA(d, kb, vb, n); ok, ov = kb.toHost(), vb.toHost(); kb.release(); vb.release()
        assert np.all(ok[1:] >= ok[:-1]); same = ok[1:] == ok[:-1]
        assert np.all(ov[1:][same] > ov[:-1][same]) and np.array_equal(k[ov], ok), (it, kind, n, algo, bits, tile, dist)
    elif kind == "compact":   # a stable partition of the keys (as int32) below / not below one of them, 8-byte values and positions along
        n = min(n, 1 << 24)
        k = k[:n]
        th = k[n // 3]
        v = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        kb = Buffer(d, n, np.int32); vb = Buffer(d, n, np.uint64); kb.write(k.view(np.int32)); vb.write(v)
        r = p.compactIf(d, kb, n, "lt", th.view(np.int32), values=vb, partition=True, indexOut=True)
        s, ok, ov, oi = int(r.count.toHost()[0]), r.items.toHost().view(np.uint32), r.values.toHost(), r.index.toHost()
        for b in (kb, vb, r.items, r.values, r.index, r.count): b.release()
        below = k.view(np.int32) < th.view(np.int32)
        order = np.concatenate([np.flatnonzero(below), np.flatnonzero(~below)])
        assert s == int(below.sum()) and np.array_equal(oi, order) and np.array_equal(ok, k[order]) and np.array_equal(ov, v[order]), (it, kind, n, dist)
    elif kind == "merge":   # two sorted parts of the keys merged, against the stable argsort of the codes of their concatenation
        mr = np.random.RandomState(args.seed + 11 * it)
        n = min(n, 1 << 24)
        na = int(mr.choice([0, 1, n // 2, n - 1, n, int(mr.randint(0, n + 1))])); nb = n - na
        dt, desc = [np.int32, np.float32][mr.randint(0, 2)], bool(mr.randint(0, 2))
        d.setParam("debug.merge_grid", int(mr.choice([0, 0, 1, 7, 300])))
        ka = Buffer(d, max(na, 1), dt); kb = Buffer(d, max(nb, 1), dt); ko = Buffer(d, n, dt)
        va = Buffer(d, max(na, 1), np.uint64); vb = Buffer(d, max(nb, 1), np.uint64); vo = Buffer(d, n, np.uint64)
        v = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        if na: ka.write(k[:na].view(dt)); va.write(v[:na]); p.sortPairs(d, ka, va, na, descending=desc)
        if nb: kb.write(k[na:n].view(dt)); vb.write(v[na:n]); p.sortPairs(d, kb, vb, nb, descending=desc)
        oi = p.mergePairs(d, ka, va, kb, vb, ko, vo, na, nb, descending=desc, indexOut=True)
        sa, sb, sva, svb = ka.toHost()[:na].view(np.uint32), kb.toHost()[:nb].view(np.uint32), va.toHost()[:na], vb.toHost()[:nb]
        ok, ov, gi = ko.toHost().view(np.uint32), vo.toHost(), oi.toHost()
        for b in (ka, kb, ko, va, vb, vo, oi): b.release()
        d.setParam("debug.merge_grid", 0)
        cat = np.concatenate([sa, sb])
        code = cat ^ np.uint32(0x80000000) if dt == np.int32 else cat ^ np.where(cat & np.uint32(0x80000000) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))
        order = np.argsort(~code if desc else code, kind="stable")
        assert np.array_equal(gi, order) and np.array_equal(ok, cat[order]) and np.array_equal(ov, np.concatenate([sva, svb])[order]), (it, kind, n, na, dt, desc, dist)
        assert np.array_equal(np.sort(ov), np.sort(v)), (it, kind, "the values are not a permutation")
    elif kind == "search":   # the bounds of needles in a sorted part of the keys, against numpy.searchsorted on the codes
        sr = np.random.RandomState(args.seed + 17 * it)
        n = min(n, 1 << 24)
        m = int(sr.choice([0, 1, 2, 4096, 4097, n // 2, int(sr.randint(0, n))])); m = min(m, n - 1); nn = n - m
        dt, desc, right = [np.int32, np.float32][sr.randint(0, 2)], bool(sr.randint(0, 2)), bool(sr.randint(0, 2))
        d.setParam("debug.search_grid", int(sr.choice([0, 0, 1, 7, 300])))
        d.setParam("debug.search_lds_keys", int(sr.choice([0, 0, 2, 3, 100])))
        ks = Buffer(d, max(m, 1), dt); kx = Buffer(d, nn, dt); po = Buffer(d, nn, np.uint32)
        x = k[m:n].copy()
        if m: x[::3] = k[:m][sr.randint(0, m, size=x[::3].size)]      # a third of the needles are in the sequence
        if m: ks.write(k[:m].view(dt)); p.sortKeys(d, ks, m, descending=desc)
        kx.write(x.view(dt))
        p.searchSorted(d, ks, kx, po, m, nn, descending=desc, right=right)
        ss, got = ks.toHost()[:m].view(np.uint32), po.toHost()
        for b in (ks, kx, po): b.release()
        d.setParam("debug.search_grid", 0); d.setParam("debug.search_lds_keys", 0)
        def code(a):
            c = a ^ np.uint32(0x80000000) if dt == np.int32 else a ^ np.where(a & np.uint32(0x80000000) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))
            return ~c if desc else c
        assert np.array_equal(got, np.searchsorted(code(ss), code(x), side="right" if right else "left").astype(np.uint32)), (it, kind, m, nn, dt, desc, right, dist)
    elif kind == "segments":   # every segment sorted on its own, against the stable lexsort on (segment, code)
        sr = np.random.RandomState(args.seed + 19 * it)
        n = min(n, 1 << 22); k = k[:n]
        top = int(sr.choice([1, 2, 33, 4096, 4097, 100000]))
        lens = np.minimum(np.floor(sr.uniform(1e-9, 1, size=n) ** -0.8), top) if sr.randint(0, 2) else sr.randint(0, top + 1, size=n)
        lens = lens.astype(np.int64); lens[sr.randint(0, n, size=n // 8)] = 0      # runs of empty segments
        S = min(int(np.searchsorted(np.cumsum(lens), n)) + 1, n); lens = lens[:S]; lens[-1] -= int(lens.sum()) - n
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        dt, desc, glob = [np.int32, np.float32][sr.randint(0, 2)], bool(sr.randint(0, 2)), bool(sr.randint(0, 2))
        bound = int(lens.max()); bound = int(sr.choice([bound, 0])) if bound <= 4096 else bound
        d.setParam("debug.sort_segments_grid", int(sr.choice([0, 0, 1, 7, 300])))
        kb = Buffer(d, n, dt); ko = Buffer(d, n, dt); ob = Buffer(d, S + 1, np.uint32); cnt = Buffer(d, 1, np.uint32)
        kb.write(k.view(dt)); ob.write(offs)
        out = p.sortSegments(d, kb, ob, S, maxSegment=bound, descending=desc, keysOut=ko, globalIndex=glob, oversizedOut=cnt)
        gi, gk, over = out.toHost().astype(np.int64), ko.toHost().view(np.uint32), int(cnt.toHost()[0])
        for b in (kb, ko, ob, cnt, out): b.release()
        d.setParam("debug.sort_segments_grid", 0)
        code = k ^ np.uint32(0x80000000) if dt == np.int32 else k ^ np.where(k & np.uint32(0x80000000) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))
        seg = np.repeat(np.arange(S), lens)
        order = np.lexsort((~code if desc else code, seg))   # stable: ties by position
        assert over == 0 and np.array_equal(gk, k[order]) and np.array_equal(gi, order if glob else order - offs[:-1].astype(np.int64)[seg]), (it, kind, n, S, top, dt, desc, glob, bound, dist)
    elif kind == "setop":   # a set operation on two sorted parts of the keys, against the oracle of the tests
        sr = np.random.RandomState(args.seed + 13 * it)
        n = min(n, 1 << 22)
        na = int(sr.choice([0, 1, n // 2, n - 1, n, int(sr.randint(0, n + 1))])); nb = n - na
        tname, desc, opname = ["i32", "f32"][sr.randint(0, 2)], bool(sr.randint(0, 2)), setop_oracle.OPS[sr.randint(0, 4)]
        dt = {"i32": np.int32, "f32": np.float32}[tname]
        k = k[:n] % np.uint32(sr.choice([1, 3, 1000, max(n // 2, 1), 1 << 31]))   # from one run to hardly a key shared
        d.setParam("debug.setop_grid", int(sr.choice([0, 0, 1, 7, 300])))
        cap = n if opname in ("union", "symmetric_difference") else na
        ka = Buffer(d, max(na, 1), dt); kb = Buffer(d, max(nb, 1), dt); ko = Buffer(d, max(cap, 1), dt)
        va = Buffer(d, max(na, 1), np.uint64); vb = Buffer(d, max(nb, 1), np.uint64); vo = Buffer(d, max(cap, 1), np.uint64)
        v = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        if na: ka.write(k[:na].view(dt)); va.write(v[:na]); p.sortPairs(d, ka, va, na, descending=desc)
        if nb: kb.write(k[na:n].view(dt)); vb.write(v[na:n]); p.sortPairs(d, kb, vb, nb, descending=desc)
        r = p.setOp(d, opname, ka, kb, ko, na, nb, descending=desc, valuesA=va, valuesB=vb, valuesOut=vo, indexOut=True)
        sa, sb, sva, svb = ka.toHost()[:na].view(np.uint32), kb.toHost()[:nb].view(np.uint32), va.toHost()[:na], vb.toHost()[:nb]
        cnt = int(r.count.toHost()[0])
        ok, ov, gi = ko.toHost().view(np.uint32)[:cnt], vo.toHost()[:cnt], r.index.toHost()[:cnt]
        for b in (ka, kb, ko, va, vb, vo, r.index, r.count): b.release()
        d.setParam("debug.setop_grid", 0)
        wi, wk, wv, wc = setop_oracle.setop_oracle(sa, sb, tname, setop_oracle.OP_IDS[opname], 1 if desc else 0, sva, svb)
        assert cnt == wc and np.array_equal(gi, wi) and np.array_equal(ok, wk) and np.array_equal(ov, wv), (it, kind, opname, n, na, tname, desc, dist)
    elif kind == "join":   # a join of two sorted parts of the keys, against the oracle of the tests
        sr = np.random.RandomState(args.seed + 23 * it)
        n = min(n, 1 << 22)
        na = int(sr.choice([1, n // 2, n - 1, n, int(sr.randint(1, n + 1))])); nb = n - na
        tname, desc, how = ["i32", "f32"][sr.randint(0, 2)], bool(sr.randint(0, 2)), join_oracle.KINDS[sr.randint(0, 4)]
        dt = {"i32": np.int32, "f32": np.float32}[tname]
        k = k[:n] % np.uint32(sr.choice([max(n // 64, 1), max(n // 2, 1), 1 << 31]))   # runs of a few dozen keys down to hardly a key shared
        d.setParam("debug.join_grid", int(sr.choice([0, 0, 1, 7, 300])))
        d.setParam("debug.search_lds_keys", int(sr.choice([0, 0, 2, 100])))
        ka = Buffer(d, na, dt); kb = Buffer(d, max(nb, 1), dt)
        ka.write(k[:na].view(dt)); p.sortKeys(d, ka, na, descending=desc)
        if nb: kb.write(k[na:n].view(dt)); p.sortKeys(d, kb, nb, descending=desc)
        sa, sb = ka.toHost()[:na].view(np.uint32), kb.toHost()[:nb].view(np.uint32)
        total = int(p.joinSorted(d, how, ka, kb, na, nb, descending=desc).count.toHost()[0])
        cap = min(int(sr.choice([total, total // 2, total + 5, 1])), 1 << 25)
        wa, wb_, wt = join_oracle.join_oracle(sa, sb, tname, join_oracle.KIND_IDS[how], 1 if desc else 0, limit=cap)
        assert total == wt, (it, kind, how, n, na, tname, desc, dist)
        if cap:
            r = p.joinSorted(d, how, ka, kb, na, nb, cap=cap, indexA=True, indexB=True, descending=desc)
            rows = min(total, cap)
            ga, gb, cnt = r.indexA.toHost()[:rows], r.indexB.toHost()[:rows], int(r.count.toHost()[0])
            for b in (r.indexA, r.indexB, r.count): b.release()
            assert cnt == wt and np.array_equal(ga, wa) and np.array_equal(gb, wb_), (it, kind, how, n, na, cap, tname, desc, dist)
        for b in (ka, kb): b.release()
        d.setParam("debug.join_grid", 0); d.setParam("debug.search_lds_keys", 0)
    elif kind == "expand":   # run-length decode of counts drawn from the keys, 8-byte values along
        sr = np.random.RandomState(args.seed + 29 * it)
        n = min(n, 1 << 21)
        counts = (k[:n] % np.uint32(sr.choice([1, 2, 5, 40]))).astype(np.uint32)
        for _ in range(int(sr.randint(0, 4))):   # stretches of runs without rows, and a few long runs
            at = int(sr.randint(0, n)); counts[at:at + int(sr.randint(1, 20000))] = 0
            counts[int(sr.randint(0, n))] = int(sr.randint(1000, 3000000))
        v = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        wr, wk, wv, total = join_oracle.expand_oracle(counts, v)
        cap = int(sr.choice([total, total // 2, total + 5, 1]))
        d.setParam("debug.join_grid", int(sr.choice([0, 0, 1, 7, 300])))
        cb = Buffer(d, n, np.uint32); vb = Buffer(d, n, np.uint64); vo = Buffer(d, max(cap, 1), np.uint64)
        cb.write(counts); vb.write(v)
        if cap:
            r = p.expandRuns(d, cb, n, cap=cap, values=vb, runOut=True, rankOut=True, valuesOut=vo)
            rows = min(total, cap)
            assert int(r.count.toHost()[0]) == total, (it, kind, n, cap, dist)
            assert np.array_equal(r.run.toHost()[:rows], wr[:rows]) and np.array_equal(r.rank.toHost()[:rows], wk[:rows]) and np.array_equal(vo.toHost()[:rows], wv[:rows]), (it, kind, n, cap, dist)
            for b in (r.run, r.rank, r.count): b.release()
        else:
            r = p.expandRuns(d, cb, n)
            assert int(r.count.toHost()[0]) == 0; r.count.release()
        for b in (cb, vb, vo): b.release()
        d.setParam("debug.join_grid", 0)
    elif kind == "hist":   # a histogram of the keys: mode, type, bins and grid knob from a generator of this iteration's own
        hr = np.random.RandomState(args.seed + 7 * it)
        n = min(n, 1 << 24)
        k = k[:n]
        wide = bool(hr.randint(0, 2))
        if wide: k = k.astype(np.uint64) * np.uint64(0x100000001) >> np.uint64(hr.randint(0, 33))
        d.setParam("debug.histogram_grid", int(hr.choice([0, 0, 1, 5, 64, 300])))
        if hr.randint(0, 2):   # range: sorted edges drawn from the keys (some repeated) and from anywhere
            tname = ["uf", "UF"][wide][hr.randint(0, 2)] if hr.randint(0, 3) else "iI"[wide]
            dt = {"u": np.uint32, "i": np.int32, "f": np.float32, "U": np.uint64, "I": np.int64, "F": np.float64}[tname]
            bins = int(hr.choice([1, 2, 17, 256, 1000, 4096]))
            e = np.concatenate([k[hr.randint(0, n, size=bins // 2 + 1)], hr.randint(0, 1 << 32, size=bins - bins // 2).astype(k.dtype) << k.dtype.type(8 * k.itemsize - 32)])
            sign = k.dtype.type(1 << (8 * k.itemsize - 1)); ones = k.dtype.type((1 << (8 * k.itemsize)) - 1)
            def code(x): return x ^ sign if tname in "iI" else x ^ np.where(x & sign != 0, ones, sign).astype(x.dtype) if tname in "fF" else x
            e = e[np.argsort(code(e), kind="stable")]
            upper = bool(hr.randint(0, 2))
            kb = Buffer(d, n, dt); eb = Buffer(d, bins + 1, dt); kb.write(k.view(dt)); eb.write(e.view(dt))
            cb = p.histogramRange(d, kb, n, eb, bins, include_upper=upper)
            got = cb.toHost()
            for b in (kb, eb, cb): b.release()
            kc, ec = code(k), code(e)
            b_of = np.searchsorted(ec, kc, side="right").astype(np.int64) - 1
            want = np.bincount(b_of[(b_of >= 0) & (b_of < bins)], minlength=bins)
            if upper:
                below = np.flatnonzero(ec[:bins] < ec[bins])
                want[below[-1] if below.size else bins - 1] += np.count_nonzero(kc == ec[bins])
            assert np.array_equal(got.astype(np.int64), want), (it, kind, "range", tname, n, bins, upper, dist)
        else:                  # bincount: keys folded so that about half of them are in range; small limits reach the sorted path
            dt = [[np.uint32, np.int32], [np.uint64, np.int64]][wide][hr.randint(0, 2)]
            bins = int(hr.choice([1, 7, 256, 8192, 8193, 100000, 1 << 20]))
            d.setParam("debug.histogram_lds_bins", int(hr.choice([0, 0, 64])))
            k = np.where(k % k.dtype.type(3) == 0, k, k % k.dtype.type(2 * bins))
            kb = Buffer(d, n, dt); kb.write(k.view(dt))
            cb = p.binCount(d, kb, n, bins)
            got = cb.toHost()
            for b in (kb, cb): b.release()
            d.setParam("debug.histogram_lds_bins", 0)
            v = k.view(dt)
            ok = (v >= 0) & (v < bins)
            assert np.array_equal(got.astype(np.int64), np.bincount(v[ok].astype(np.int64), minlength=bins)), (it, kind, "bincount", dt, n, bins, dist)
        d.setParam("debug.histogram_grid", 0)
    elif kind == "soaw":   # wide values / 64-bit keys on separate arrays (adlhip_radix_sort_soa): index sort + gather
        n = min(n, 1 << 23)
        k = k[:n]
        kd = np.uint64 if it % 2 else np.uint32
        vd = [np.uint64, np.uint32, np.dtype([("a", "<u8"), ("b", "<u8")])][it % 3]
        keys = k.astype(np.uint64) * np.uint64(0x100000001) >> np.uint64(it % 29) if kd == np.uint64 else k
        vals = np.zeros(n, dtype=vd)
        vals.view(np.uint32).reshape(n, -1)[:, 0] = np.arange(n, dtype=np.uint32)
        kb = Buffer(d, n, kd); vb = Buffer(d, n, vd); kb.write(keys); vb.write(vals)
        p.radixSortSoA(d, kb, vb, n); ok, ov = kb.toHost(), vb.toHost(); kb.release(); vb.release()
        idx = ov.view(np.uint32).reshape(n, -1)[:, 0].astype(np.int64)
        assert np.all(ok[1:] >= ok[:-1]); same = ok[1:] == ok[:-1]
        assert np.all(idx[1:][same] > idx[:-1][same]) and np.array_equal(keys[idx], ok), (it, kind, n, kd, vd, dist)
    else:
        k64 = oracle.keys_u64(n, seed=it)
        if dist == "lowbits": k64 &= np.uint64(0xffffff)
        elif dist == "shifted": k64 >>= np.uint64(2 * shift)
        elif dist == "fewvals": k64 = (k64 % np.uint64(7)) * np.uint64(0x0101010101010101)
        b = Buffer(d, n, np.uint64); b.write(k64); p.radixSort64(d, b, n); out = b.toHost(); b.release()
        assert np.all(out[1:] >= out[:-1]) and checks(out) == checks(k64), (it, kind, n, algo, bits, tile, dist)
    elems += n
    if time.time() - t_mark > 60:   # a sign of life for the runner
        t_mark = time.time(); print("... %d sorts, %.0f M elements" % (it, elems / 1e6), flush=True)
print("stress ok: %d sorts, %.1f M elements, %.0f s, no mismatch, no look-back fault, %d LDS-order self-tests beside running sorts: 0 mismatches"
      % (it, elems / 1e6, args.seconds, selftests))
print("safety net of the large sort: ran %d times, %d of them sorted by counting" % (d.getParam("stat.net_runs"), d.getParam("stat.net_counting")))
p.close(); DeviceUtils.deallocate(d); DeviceUtils.deallocate(d2)
