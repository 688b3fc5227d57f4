"""The typed sorts on value-shaped keys, per size class of the pair sort underneath (tests/typed_shapes.py has the inputs and the reference).

Every typed entry point that returns an order runs the stable {32 key bits, index} pair sort once per key dword (primitives.hip
typed_index_sort): 8-byte keys get two runs, low dword first, and the second must be stable on the permuted output of the first.  Each
run picks its size class by n -- one workgroup up to 16384 pairs, the mid-size form up to 1 Mi, the large stable form above -- and its
safety net by what its dword looks like.  Real int64 / float64 data makes the two dwords of a key extreme in opposite ways, so one typed
sort runs a friendly and a hostile pair sort back to back on one handle.  Here: every case x both orders x a ladder of sizes on the class
edges, bit for bit against numpy; the kernels and the nets that ran, asserted; the large form and its nets at small n; unique, reduce by
key and top-k once each on such keys; and the mid-size form's asynchronous hints, which must not change a result.

One handle serves the whole module with default knobs, so that hints and handle state carry from case to case as they would for a user.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from test_gpu_parity import LARGE_PAIRS, _profiled
from test_gpu_typed_sort import Guarded, argsort, guard_of, lib_err, random_bits, scratch_sizes, sort_keys, sort_pairs, values_for
from typed_shapes import ASC, BY_NAME, CASES, DESC, TABLE8, encoded_dwords, expected_perm, shape

pytestmark = pytest.mark.gpu

ORDER_IDS = ["asc", "desc"]
SEED = 7
# the last one-workgroup size, the first mid size, a mid size, the last mid size for 8-byte elements (kMidMaxE64), the first large size
# (kMsd2sAutoMin + 1) and one beyond
LADDER = [16384, 16385, 300_007, 1 << 20, (1 << 20) + 1, (2 << 20) + 5]
N_TOP = LADDER[-1]
ITEMS = [(name, case) for name in CASES for case in CASES[name]]
ITEM_IDS = ["%s-%s" % nc for nc in ITEMS]

SMALL = {"small_sort_e64"}
MID3 = {"mid_prep_e64", "onesweep_e64_8b", "segment_sort_e64"}
TYPED = {"typed_pack_index_k32", "typed_pack_index_k64", "typed_repack_high", "typed_gather"}


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    DeviceUtils.deallocate(d)


def net_stats(d):
    return d.getParam("stat.net_runs"), d.getParam("stat.net_counting")


# ---------------------------------------------------------------------------------------------
# a. every case x both orders x the size ladder
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,case", ITEMS, ids=ITEM_IDS)
def test_every_case_on_the_size_ladder(dev, name, case, order):
    kt = BY_NAME[name][1]
    for n in LADDER:
        x = shape(name, case, n, SEED)
        perm = expected_perm(x, name, order)
        want = x[perm]
        idx, ks = argsort(dev, kt, order, x, True)   # (asserts the input intact and the guards behind every buffer)
        assert np.array_equal(idx, perm.astype(np.uint32)), (name, case, n, "argsort: index")
        assert np.array_equal(ks, want), (name, case, n, "argsort: keys")
        v = values_for(n, 8)
        gk, gv = sort_pairs(dev, kt, order, x, v)
        assert np.array_equal(gk, want), (name, case, n, "pairs: keys")
        assert np.array_equal(gv, v[perm]), (name, case, n, "pairs: values")
        assert np.array_equal(sort_keys(dev, kt, order, x), want), (name, case, n, "keys only")
        assert dev.getParam("debug.idle_dirty") == 0, (name, case, n)
    DeviceUtils.waitForCompletion(dev)   # adlhip_sync: no device-side fault


# ---------------------------------------------------------------------------------------------
# b. the paths are asserted, not assumed
# ---------------------------------------------------------------------------------------------
def sort_kernels(prof):
    """the launches of the pair sort among a typed call's: {kernel name: launches}"""
    return {k: c for k, (c, _) in prof.items() if k not in TYPED}


def test_size_classes_show_in_the_kernel_names_once_per_dword(dev):
    """Friendly keys (uniform bit patterns) of 4 and of 8 bytes at the class edges: the one-workgroup sort alone at 16384, the mid-size
    form's three launches at 16385 and at 1 Mi ("sort.mid" = 3: the form is forced, no hint decides), the large stable form at
    1 Mi + 1.  8-byte keys show the same kernels with twice the launches -- one pair sort per dword -- and typed_repack_high once."""
    try:
        for n, knobs, names in ((16384, {}, SMALL), (16385, {"sort.mid": 3}, MID3), (1 << 20, {"sort.mid": 3}, MID3),
                                ((1 << 20) + 1, {}, LARGE_PAIRS)):
            for k, v in knobs.items():
                dev.setParam(k, v)
            launches = {}
            for name in ("i32", "i64"):
                _, kt, _, udt = BY_NAME[name]
                x = random_bits(udt, n, 100 + kt)
                perm = expected_perm(x, name, ASC)
                (idx, ks), prof = _profiled(dev, lambda: argsort(dev, kt, ASC, x, True))
                assert np.array_equal(idx, perm.astype(np.uint32)) and np.array_equal(ks, x[perm]), (name, n)
                launches[name] = sort_kernels(prof)
                assert set(launches[name]) == set(names), (name, n, prof)
                typed = {k: prof[k][0] for k in prof if k in TYPED}
                if name == "i32":
                    assert typed == {"typed_pack_index_k32": 1, "typed_gather": 1}, (n, prof)
                else:
                    assert typed == {"typed_pack_index_k64": 1, "typed_repack_high": 1, "typed_gather": 1}, (n, prof)
            assert launches["i64"] == {k: 2 * c for k, c in launches["i32"].items()}, (n, launches)
            dev.setParam("sort.mid", 1)
    finally:
        dev.setParam("sort.mid", 1)
    assert dev.getParam("debug.idle_dirty") == 0


NONE, DICT, LSD = "no net", "dictionary", "LSD net"
OUTCOME = {(0, 0): NONE, (1, 1): DICT, (1, 0): LSD}
CONST = np.uint64(0x5a5a5a5a)


def test_net_outcomes_per_dword_of_the_eight_byte_table(dev):
    """Which safety net each dword of the 8-byte table sends the large pair sort to at n = 2 Mi + 5, read off "stat.net_runs" /
    "stat.net_counting".  One typed call runs both pair sorts, so each dword is isolated in a uint64 key whose other dword is constant:
    the constant dword's sort takes the dictionary pass (asserted first, on keys that are constant in both), what is left of the
    counters' step is the outcome of the dword under test.  A low dword is then sorted exactly as in its case; a high dword on the
    same keys in input order (its case hands them over permuted by the low dword's sort).  All three outcomes -- no net, the
    dictionary pass (net_counting + 1), the LSD net (net_runs + 1 alone) -- must be seen for a low and for a high dword.

    The case itself, sorted through its own type, must then step the counters by what its two dwords take one by one.

    Observed on the MI355X (case: low dword | high dword):
        int64 uniform in [-1000, 1000]    LSD net    | dictionary
        int64 ids 1.7e18 + 1000 i         LSD net    | dictionary     (distinct and ascending, but under half of the top bytes)
        int64 multiples of 2^32           dictionary | LSD net
        float64 standard normal           no net     | LSD net
        float64 converted from float32    dictionary | LSD net
        float64 whole numbers 0..999      dictionary | LSD net
        float64, 30 % one NaN pattern     LSD net    | LSD net
        uint64 uniform bits (added)       no net     | no net         (no row of the table has a high dword that fits the slabs)
    """
    n = N_TOP
    kt = BY_NAME["u64"][1]

    def step(keys):
        before = net_stats(dev)
        perm = expected_perm(keys, "u64", ASC)
        idx, ks = argsort(dev, kt, ASC, keys, True)
        assert np.array_equal(idx, perm.astype(np.uint32)) and np.array_equal(ks, keys[perm])
        after = net_stats(dev)
        return after[0] - before[0], after[1] - before[1]

    assert step(np.full(n, (CONST << np.uint64(32)) | CONST, dtype=np.uint64)) == (2, 2), "a constant dword takes the dictionary pass"
    rows = [(name, case, shape(name, case, n, SEED)) for name, case in TABLE8]
    rows.append(("u64", "uniform bits", random_bits(np.uint64, n, 55)))
    seen = {"lo": set(), "hi": set()}
    table = []
    for name, case, x in rows:
        lo, hi = encoded_dwords(x, name)
        out = {}
        for which, d in (("lo", lo), ("hi", hi)):
            d = d.astype(np.uint64)
            keys = (CONST << np.uint64(32)) | d if which == "lo" else (d << np.uint64(32)) | CONST
            runs, counting = step(keys)
            assert (runs - 1, counting - 1) in OUTCOME, (name, case, which, runs, counting)
            out[which] = OUTCOME[(runs - 1, counting - 1)]
            seen[which].add(out[which])
        # the case itself, through its own type: as many nets as its dwords take one by one
        before = net_stats(dev)
        perm = expected_perm(x, name, ASC)
        idx, _ = argsort(dev, BY_NAME[name][1], ASC, x, False)
        assert np.array_equal(idx, perm.astype(np.uint32)), (name, case)
        after = net_stats(dev)
        whole = (after[0] - before[0], after[1] - before[1])
        both = list(out.values())
        assert whole == (sum(o != NONE for o in both), sum(o == DICT for o in both)), (name, case, out, whole)
        table.append("%s %s: %s | %s; the typed sort: net_runs + %d, net_counting + %d" % (name, case, out["lo"], out["hi"], whole[0], whole[1]))
    print("\n".join(table))
    for which in ("lo", "hi"):
        assert seen[which] == {NONE, DICT, LSD}, (which, seen[which], table)
    assert dev.getParam("debug.idle_dirty") == 0
    DeviceUtils.waitForCompletion(dev)


# ---------------------------------------------------------------------------------------------
# c. the large pair sort and its nets at small n
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40_000, 300_007])
def test_large_pair_sort_and_its_nets_at_small_n(dev, n):
    """"sort.msd2" = 2 lets pairs take the large stable form from 16385 elements (kMsd2Min) -- with "sort.mid" = 0, or the mid-size form,
    which is asked first up to 1 Mi pairs, would take them.  Below the one-sweep scratch the net runs coop_lsd_sort instead of
    coop_onesweep_sort, a form the typed layer reaches in no other way.  The 8-byte table, argsort, both orders; the scratch is
    queried after the knobs are set (argsort() does), and the kernels that ran are the large form's."""
    dev.setParam("sort.msd2", 2)
    dev.setParam("sort.mid", 0)
    try:
        for name, case in TABLE8:
            kt = BY_NAME[name][1]
            x = shape(name, case, n, SEED)
            for order in (ASC, DESC):
                perm = expected_perm(x, name, order)
                before = net_stats(dev)
                (idx, ks), prof = _profiled(dev, lambda: argsort(dev, kt, order, x, True))
                after = net_stats(dev)
                assert np.array_equal(idx, perm.astype(np.uint32)), (name, case, order, "index")
                assert np.array_equal(ks, x[perm]), (name, case, order, "keys")
                ran = sort_kernels(prof)
                # (a sort whose net ran shows no finish: its segments are empty)
                assert LARGE_PAIRS - {"segment_sort_wave_e64"} <= set(ran) <= LARGE_PAIRS, (name, case, prof)
                assert ran["msd2s_prep"] == 2 and prof["typed_repack_high"][0] == 1, (name, case, prof)
                # the nets are reached at this size too: one value on a third of the keys cannot fit a slab and has too many
                # neighbours for the dictionary, a constant dword cannot fit either and is the dictionary's
                if case == "nan30":
                    assert after[0] - before[0] >= 1, (n, order, before, after)
                if case == "mult_2p32":
                    assert after[1] - before[1] >= 1, (n, order, before, after)
        assert dev.getParam("debug.idle_dirty") == 0
        DeviceUtils.waitForCompletion(dev)
    finally:
        dev.setParam("sort.msd2", 1)
        dev.setParam("sort.mid", 1)


# ---------------------------------------------------------------------------------------------
# d. downstream of the index sort, once each
# ---------------------------------------------------------------------------------------------
N_DOWN = (1 << 20) + 77


def test_unique_with_inverse_and_first_index_on_small_int64_values(dev):
    x = shape("i64", "uniform_pm1000", N_DOWN, SEED).view(np.int64)
    want_u, want_first, want_inv, want_counts = np.unique(x, return_index=True, return_inverse=True, return_counts=True)
    p = Pprims()
    kb = Buffer(dev, N_DOWN, np.int64)
    r = None
    try:
        kb.write(x)
        r = p.unique(dev, kb, N_DOWN, counts=True, firstIndex=True, inverse=True)
        count = int(r.count.toHost()[0])
        assert count == want_u.size == 2001
        assert np.array_equal(r.unique.toHost()[:count], want_u)
        assert np.array_equal(r.counts.toHost()[:count], want_counts.astype(np.uint32))
        assert np.array_equal(r.firstIndex.toHost()[:count], want_first.astype(np.uint32))
        assert np.array_equal(r.inverse.toHost(), want_inv.reshape(-1).astype(np.uint32))
        assert np.array_equal(kb.toHost(), x), "unique changed its input"
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for b in (kb,) + tuple(b for b in (r or ()) if b is not None):
            b.release()
        p.close()


def test_reduce_by_key_sums_on_whole_number_float64_keys(dev):
    bits = shape("f64", "whole", N_DOWN, SEED)
    keys = bits.view(np.float64)
    vals = (np.arange(N_DOWN, dtype=np.int64) * 2654435761) % 2001 - 1000
    want_sum = np.zeros(1000, np.int64)
    np.add.at(want_sum, keys.astype(np.int64), vals)
    want_counts = np.bincount(keys.astype(np.int64), minlength=1000)
    assert want_counts.min() > 0   # all of 0..999 occur: key r is the whole number r
    p = Pprims()
    kb, vb = Buffer(dev, N_DOWN, np.float64), Buffer(dev, N_DOWN, np.int64)
    r = None
    try:
        kb.write(keys)
        vb.write(vals)
        r = p.reduceByKey(dev, kb, vb, N_DOWN, op="sum", counts=True)
        count = int(r.count.toHost()[0])
        assert count == 1000
        assert np.array_equal(r.unique.toHost()[:count], np.arange(1000, dtype=np.float64))
        assert np.array_equal(r.reduced.toHost()[:count], want_sum)
        assert np.array_equal(r.counts.toHost()[:count], want_counts.astype(np.uint32))
        assert np.array_equal(kb.toHost().view(np.uint64), bits) and np.array_equal(vb.toHost(), vals), "reduceByKey changed its input"
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for b in (kb, vb) + tuple(b for b in (r or ()) if b is not None):
            b.release()
        p.close()


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
def test_topk_by_full_argsort_on_float64_with_one_nan_pattern(dev, order):
    bits = shape("f64", "nan30", N_DOWN, SEED)
    k = N_DOWN // 2
    perm = expected_perm(bits, "f64", order)[:k]
    p = Pprims()
    kb, ko = Buffer(dev, N_DOWN, np.float64), Buffer(dev, k, np.float64)
    ib = None
    dev.setParam("topk.algo", 0)
    try:
        kb.write(bits.view(np.float64))
        ib = p.topk(dev, kb, N_DOWN, k, descending=order == DESC, keysOut=ko)
        assert np.array_equal(ib.toHost(), perm.astype(np.uint32))
        assert np.array_equal(ko.toHost().view(np.uint64), bits[perm])
        assert np.array_equal(kb.toHost().view(np.uint64), bits), "topk changed its input"
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.algo", -1)
        for b in (kb, ko, ib):
            if b is not None:
                b.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# e. hints do not change results
# ---------------------------------------------------------------------------------------------
def test_mid_size_hints_raised_by_one_dword_do_not_change_the_other_sorts(dev):
    """The mid-size form steers by reports of its own earlier sorts that the host reads without synchronising (choose_mid_form: "only
    speed depends on any of this").  float64 keys converted from float32 (16 low dwords, high dwords under one top byte) and uniform
    uint64 keys alternate at n = 300007, eight argsorts enqueued without a host read in between: each dword wants the opposite hint,
    and the hint one sort raises may arrive during any later one.  Every result is bit-exact."""
    n = 300_007
    lib = _lib.load()
    inputs = [("f64", shape("f64", "from_f32", n, SEED)), ("u64", random_bits(np.uint64, n, 66))]
    want = [expected_perm(x, name, ASC) for name, x in inputs]
    wb = max(scratch_sizes(dev, BY_NAME[name][1], 2, 0, n)[2] for name, _ in inputs)
    g = guard_of(np.uint64)
    src = [Guarded(dev, x, guard_bytes=g, seed=30 + i) for i, (_, x) in enumerate(inputs)]
    outs = [(Guarded(dev, nbytes=8 * n, guard_bytes=g, seed=40 + i), Guarded(dev, nbytes=4 * n, guard_bytes=guard_of(np.uint32), seed=50 + i))
            for i in range(8)]
    w = Guarded(dev, nbytes=max(wb, 16), seed=60)
    try:
        for i, (ko, io) in enumerate(outs):
            name = inputs[i % 2][0]
            rc = lib.adlhip_argsort_typed(dev._h, BY_NAME[name][1], ASC, src[i % 2].ptr(), ko.ptr(), io.ptr(), w.ptr(), wb, n)
            assert rc == 0, lib_err()
        for i, (ko, io) in enumerate(outs):   # the first host read: everything above was enqueued back to back
            x, perm = inputs[i % 2][1], want[i % 2]
            assert np.array_equal(io.read(np.uint32)[:n], perm.astype(np.uint32)), i
            assert np.array_equal(ko.read(np.uint64)[:n], x[perm]), i
        w.check_guard()
        for s, (_, x) in zip(src, inputs):
            assert np.array_equal(s.read(np.uint64), x), "argsort changed its input"
        assert dev.getParam("debug.idle_dirty") == 0
        DeviceUtils.waitForCompletion(dev)
    finally:
        for b in src + [b for pair in outs for b in pair] + [w]:
            b.release()
