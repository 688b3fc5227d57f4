"""Set operations on sorted sequences on the GPU (include/adlhip.h "set operations on sorted sequences";
oclradixsort_amd/csrc/setop_kernels.hpp; Pprims.setOp; TorchSorter.intersect / union / difference / symmetric_difference).

The oracle is tests/setop_oracle.py (numpy: the stable merge order of A || B with the keep rules of the header applied;
tests/test_setop_api.py checks it against a Counter multiset and thrust's two-pointer loops).  Every case is compared bit for bit: the
count word, and the first S elements of every output.

Every output is sized exactly its capacity (na for intersection and difference, na + nb for union and symmetric difference),
prefilled with sentinels and read back whole: elements [S, cap) and the guard bytes behind cap must be untouched.  Every input and
the work buffer (sized exactly the reported bytes and prefilled with junk) carry guard bytes too, and the inputs are compared with
their originals afterwards.  The handle's device state is idle after each case.

T is the tile of the set operations: 2048 elements of the merged order.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from setop_oracle import (ASC, BY_NAME, DESC, DIFFERENCE, INTERSECTION, OPS, SPECIALS, SYMMETRIC_DIFFERENCE, TYPE_IDS, UNION, capacity, codes,
                          is_sorted, setop_oracle, sort_bits)
from test_gpu_merge import Padded
from test_gpu_reduce import Guarded, lib_err, random_bits, sentinels

pytestmark = pytest.mark.gpu

T = 2048
ALL_OPS = (INTERSECTION, UNION, DIFFERENCE, SYMMETRIC_DIFFERENCE)
GRIDS = [0, 1, 3]
ORDERS = [ASC, DESC]
SENTINELS = 64
UDT = {0: None, 4: np.uint32, 8: np.uint64}
COUNT_SENTINEL = np.array([0xdeadbeef], np.uint32)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.setop_grid", 0)
    DeviceUtils.deallocate(d)


def scratch_bytes(dev, key_type, value_bytes, na, nb):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_set_op_scratch_bytes(dev._h, key_type, value_bytes, na, nb, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Case:
    """the device side of a series of set operations on the same inputs: guarded inputs, for each of the two capacities (na; na + nb)
    sentinel-filled outputs of exactly that many elements, a guarded count word, a work buffer of exactly the reported bytes prefilled
    with junk.  outs: {name: dtype}"""

    def __init__(self, dev, kname, a, b, va=None, vb=None, outs=None, off=(0, 0), fill=0xff):
        self.dev, self.kname, self.a, self.b, self.va, self.vb = dev, kname, a, b, va, vb
        self.na, self.nb, self.n = a.size, b.size, a.size + b.size
        self.vbytes = va.dtype.itemsize if va is not None else 0
        self.ins = {"a": Padded(dev, a, off[0], 5), "b": Padded(dev, b, off[1], 6)}
        if va is not None:
            self.ins["va"] = Padded(dev, va, off[0], 7)
            self.ins["vb"] = Padded(dev, vb, off[1], 8)
        self.sent, self.dout = {}, {}
        for both in (False, True):
            cap = self.n if both else self.na
            for i, (k, dt) in enumerate(outs.items()):
                s = sentinels(dt, cap, 0xa5a5a5a5a5a5a5a5 + 77 * i + both)
                self.sent[(both, k)] = s
                self.dout[(both, k)] = Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=20 + i)
        self.count = Guarded(dev, COUNT_SENTINEL, guard_bytes=64, seed=3)
        self.work = Guarded(dev, nbytes=scratch_bytes(dev, BY_NAME[kname][1], self.vbytes, self.na, self.nb), seed=9, fill=fill)

    def reset(self):
        for k, s in self.sent.items():
            if s.size:
                self.dout[k].buf.write(s.view(np.uint8))
        self.count.buf.write(COUNT_SENTINEL.view(np.uint8))

    def inp(self, name):
        return self.ins[name].ptr() if name in self.ins else None

    def out(self, op, name):
        k = (op in (UNION, SYMMETRIC_DIFFERENCE), name)
        return self.dout[k].ptr() if k in self.dout else None

    def call(self, order, op, **over):
        """adlhip_set_op_typed on the case's buffers; over: arguments that replace them"""
        arg = dict(key_type=BY_NAME[self.kname][1], order=order, op=op, a=self.inp("a"), va=self.inp("va"), na=self.na, b=self.inp("b"),
                   vb=self.inp("vb"), nb=self.nb, value_bytes=self.vbytes, ko=self.out(op, "keys"), vo=self.out(op, "vals"),
                   xo=self.out(op, "index"), num=self.count.ptr(), work=self.work.ptr(), work_bytes=self.work.nbytes)
        arg.update(over)
        return _lib.load().adlhip_set_op_typed(self.dev._h, arg["key_type"], arg["order"], arg["op"], arg["a"], arg["va"], arg["na"], arg["b"],
                                               arg["vb"], arg["nb"], arg["value_bytes"], arg["ko"], arg["vo"], arg["xo"], arg["num"],
                                               arg["work"], arg["work_bytes"])

    def read(self):
        """the count word and every output, whole; the guards behind every buffer checked"""
        got = {k: g.read(self.sent[k].dtype) for k, g in self.dout.items()}
        self.work.check_guard()
        return int(self.count.read(np.uint32)[0]), got

    def inputs_unchanged(self):
        for k, p in self.ins.items():
            assert p.unchanged(), "input %s was changed" % k

    def check(self, op, exp, count, what):
        """exp: {name: the S expected elements}; the outputs of the other capacity must be untouched altogether"""
        s, got = self.read()
        assert s == count, "%s: the count word says %d, expected %d" % (what, s, count)
        mine = op in (UNION, SYMMETRIC_DIFFERENCE)
        for (both, k), g in got.items():
            sent = self.sent[(both, k)]
            if both != mine:
                assert np.array_equal(g, sent), "%s: an output that was not passed was written" % what
                continue
            e = exp[k]
            assert e.size == s
            if not np.array_equal(g[:s], e):
                bad = np.flatnonzero(g[:s] != e)
                raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                    what, k, bad.size, s, bad[0], int(g[bad[0]]), int(e[bad[0]])))
            assert np.array_equal(g[s:], sent[s:]), "%s: %s was written at S = %d or beyond" % (what, k, s)
        self.inputs_unchanged()
        assert self.dev.getParam("debug.idle_dirty") == 0

    def untouched(self):
        s, got = self.read()
        assert s == COUNT_SENTINEL[0], "the count word was written"
        for k, g in got.items():
            assert np.array_equal(g, self.sent[k]), "%s was written" % (k,)
        self.inputs_unchanged()

    def release(self):
        for b in list(self.ins.values()) + list(self.dout.values()) + [self.work, self.count]:
            b.release()


def run_setop(dev, kname, a, b, va=None, vb=None, form=("keys", "vals", "index"), orders=(ASC,), grids=(0,), ops=ALL_OPS, off=(0, 0),
              fill=0xff, presorted=False):
    """adlhip_set_op_typed on a and b, each sorted here (stably, values along) in every order asked, for every op and grid, with every
    check of the memory contract.  Returns {(order, op): the oracle's (index, keys, values, count)}"""
    form = tuple(k for k in form if k != "vals" or va is not None)
    res = {}
    for order in orders:
        if presorted:
            sa, sb, sva, svb = a, b, va, vb
        else:
            pa, pb = np.argsort(codes(a, kname, order), kind="stable"), np.argsort(codes(b, kname, order), kind="stable")
            sa, sb = a[pa], b[pb]
            sva, svb = (va[pa], vb[pb]) if va is not None else (None, None)
        assert is_sorted(sa, kname, order) and is_sorted(sb, kname, order)
        odt = {k: {"keys": sa.dtype, "vals": sva.dtype if sva is not None else None, "index": np.uint32}[k] for k in form}
        c = Case(dev, kname, sa, sb, sva, svb, odt, off=off, fill=fill)
        try:
            for op in ops:
                index, keys, vals, count = setop_oracle(sa, sb, kname, op, order, sva, svb)
                res[(order, op)] = (index, keys, vals, count)
                exp = {k: {"keys": keys, "vals": vals, "index": index}[k] for k in form}
                for grid in grids:
                    dev.setParam("debug.setop_grid", grid)
                    c.reset()
                    what = "%s %s order %d %s na %d nb %d value_bytes %d grid %d off %s" % (OPS[op], kname, order, "+".join(form), sa.size,
                                                                                           sb.size, c.vbytes, grid, off)
                    rc = c.call(order, op)
                    assert rc == 0, what + ": " + lib_err()
                    c.check(op, exp, count, what)
        finally:
            dev.setParam("debug.setop_grid", 0)
            c.release()
    return res


def _form(form):
    """("keys", "vals8", "index") -> (the outputs' names, the values' width)"""
    vb = 0
    names = []
    for k in form:
        if k.startswith("vals"):
            vb = int(k[4:])
            names.append("vals")
        else:
            names.append(k)
    return tuple(names), vb


# ---------------------------------------------------------------------------------------------
# sizes x grids x ops
# ---------------------------------------------------------------------------------------------
TOTALS = [0, 1, T - 1, T, T + 1, 3 * T - 1, 3 * T + 1]


def _splits(n):
    return sorted({(0, n), (n, 0), (min(1, n), n - min(1, n)), (n // 2, n - n // 2)})


@pytest.mark.parametrize("n", TOTALS)
def test_sizes_grids_and_ops(dev, n):
    rng = np.random.default_rng(1000 + n)
    for na, nb in _splits(n):
        # a third as many distinct keys as elements: duplicates inside an input and across the inputs
        a, b = (rng.integers(0, n // 3 + 2, size=m).astype(np.uint32) for m in (na, nb))
        run_setop(dev, "i32", a, b, random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng), grids=GRIDS)
    na, nb = _splits(n)[-1]
    a, b = (rng.integers(0, n // 3 + 2, size=m).astype(np.uint64) for m in (na, nb))
    run_setop(dev, "f64", a, b, form=("keys", "index"), orders=(DESC,), grids=GRIDS)


def test_more_tiles_than_one_chunk_on_the_default_grid(dev):
    """8 workgroups per CU take one tile each up to 8 x CUs tiles; beyond that a chunk is several tiles"""
    tiles = 8 * int(dev.info.compute_units) + 5
    na = nb = tiles * T // 2 + 3
    rng = np.random.default_rng(23)
    a, b = (rng.integers(0, na, size=m).astype(np.uint32) for m in (na, nb))
    run_setop(dev, "u32", a, b, form=("keys",), ops=(INTERSECTION, SYMMETRIC_DIFFERENCE))


# ---------------------------------------------------------------------------------------------
# runs against tile edges
# ---------------------------------------------------------------------------------------------
X = 0x40000000


def _edge_cases():
    u = np.uint32
    lows = lambda k: np.arange(k, dtype=u)                         # noqa: E731  (distinct keys below X)
    highs = lambda k, at=1: np.arange(k, dtype=u) * u(2) + u(X + at)   # noqa: E731  (distinct keys above X; odd or even)
    run = lambda k: np.full(k, X, u)                               # noqa: E731
    cases = {
        "all_one_key_5000_3000": (run(5000), run(3000)),
        "all_one_key_3000_5000": (run(3000), run(5000)),
        "three_keys_three_tiles": None,
        # A holds one copy of X in the first tile; B's run of X starts there and ends two tiles later
        "b_run_over_three_tiles": (np.concatenate([lows(T - 10), run(1), highs(20)]), np.concatenate([run(2 * T + 50), highs(5, 2)])),
        # the mirror: A's run crosses two boundaries, B holds one copy behind it
        "a_run_over_three_tiles": (np.concatenate([lows(7), run(2 * T + 50), highs(5, 2)]), np.concatenate([lows(T - 30), run(1), highs(20)])),
        "disjoint_a_below_b": (lows(2 * T + 3), highs(T + 9)),
        "disjoint_b_below_a": (highs(T + 9), lows(2 * T + 3)),
        "strictly_interleaved": (np.arange(T + 700, dtype=u) * u(2), np.arange(T + 703, dtype=u) * u(2) + u(1)),
        "pairs_of_twins": (np.arange(T + 700, dtype=u) * u(3), np.arange(T + 703, dtype=u) * u(3)),
    }
    # A's part of the run of X ends on the last output of the first tile, B's part starts on the first output of the second; +-1
    for shift in (-1, 0, 1):
        cases["run_split_at_the_boundary_%+d" % shift] = (np.concatenate([lows(T - 5 + shift), run(5), highs(30)]),
                                                          np.concatenate([run(7), highs(40, 2)]))
        # the same with more of X in A than in B, and the run's end on the boundary of the second tile
        cases["run_ends_at_the_boundary_%+d" % shift] = (np.concatenate([lows(2 * T - 20 + shift), run(13)]),
                                                         np.concatenate([run(7), highs(40, 2)]))
    rng = np.random.default_rng(5)
    cases["three_keys_three_tiles"] = (np.sort(rng.integers(0, 3, size=T + T // 2).astype(u)), np.sort(rng.integers(0, 3, size=T + T // 2).astype(u)))
    return cases


EDGE_CASES = _edge_cases()


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_runs_against_tile_edges(dev, name):
    a, b = EDGE_CASES[name]
    rng = np.random.default_rng(len(name))
    va, vb = random_bits(np.uint32, a.size, rng), random_bits(np.uint32, b.size, rng)
    res = run_setop(dev, "u32", a, b, va, vb, orders=ORDERS, grids=(0, 1, 3))
    run_setop(dev, "u64", a.astype(np.uint64) << np.uint64(20), b.astype(np.uint64) << np.uint64(20), form=("index",), grids=(0, 3))
    if name == "all_one_key_5000_3000":      # m = 5000, n = 3000: the first 3000 of A; all of A; the last 2000 of A, twice
        exp = {INTERSECTION: np.arange(3000), UNION: np.arange(5000), DIFFERENCE: np.arange(3000, 5000), SYMMETRIC_DIFFERENCE: np.arange(3000, 5000)}
        for op, idx in exp.items():
            assert np.array_equal(res[(ASC, op)][0], idx.astype(np.uint32))
    if name == "all_one_key_3000_5000":      # m = 3000, n = 5000: all of A; A and the last 2000 of B; nothing; the last 2000 of B
        exp = {INTERSECTION: np.arange(3000), UNION: np.concatenate([np.arange(3000), np.arange(6000, 8000)]), DIFFERENCE: np.arange(0),
               SYMMETRIC_DIFFERENCE: np.arange(6000, 8000)}
        for op, idx in exp.items():
            assert np.array_equal(res[(DESC, op)][0], idx.astype(np.uint32))


def test_a_and_b_the_same_array(dev):
    """A == B, the same pointer: intersection = union = A, difference and symmetric difference empty"""
    rng = np.random.default_rng(72)
    h = 2 * T + 5
    a = sort_bits(rng.integers(0, 500, size=h).astype(np.uint64), "i64", DESC)
    c = Case(dev, "i64", a, a, None, None, {"keys": np.uint64, "index": np.uint32})
    try:
        for op in ALL_OPS:
            index, keys, _, count = setop_oracle(a, a, "i64", op, DESC)
            assert count == (h if op in (INTERSECTION, UNION) else 0)
            if count:
                assert np.array_equal(index, np.arange(h, dtype=np.uint32))
            for grid in (0, 1):
                dev.setParam("debug.setop_grid", grid)
                c.reset()
                assert c.call(DESC, op, b=c.inp("a")) == 0, lib_err()
                c.check(op, {"keys": keys, "index": index}, count, "B is A, %s" % OPS[op])
    finally:
        dev.setParam("debug.setop_grid", 0)
        c.release()


# ---------------------------------------------------------------------------------------------
# types, orders, ops, forms
# ---------------------------------------------------------------------------------------------
FORMS = [("keys",), ("index",), ("keys", "vals4"), ("keys", "vals8", "index")]


@pytest.mark.parametrize("order", ORDERS, ids=["asc", "desc"])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_every_key_type_order_op_and_form_with_special_patterns(dev, kname, order):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    na, nb = T + 300, T + 500
    rng = np.random.default_rng(400 + BY_NAME[kname][1])
    pool = np.concatenate([random_bits(udt, 300, rng), SPECIALS[w]])          # both inputs draw from one pool: shared keys, duplicates
    a, b = pool[rng.integers(0, pool.size, size=na)], pool[rng.integers(0, pool.size, size=nb)]
    for x in (a, b):                                      # specials that repeat, in both inputs (+-0, +-inf, NaN payloads)
        x[rng.integers(0, x.size, size=x.size // 3)] = SPECIALS[w][rng.integers(0, SPECIALS[w].size, size=x.size // 3)]
    for form in FORMS:
        names, vbytes = _form(form)
        va = random_bits(UDT[vbytes], na, rng) if vbytes else None
        vb = random_bits(UDT[vbytes], nb, rng) if vbytes else None
        run_setop(dev, kname, a, b, va, vb, form=names, orders=(order,), grids=(0, 1) if form == FORMS[-1] else (0,))


# ---------------------------------------------------------------------------------------------
# alignment and aliasing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [(1, 0), (0, 3), (3, 1)], ids=lambda o: "%d_%d" % o)
@pytest.mark.parametrize("kname,vbytes", [("f32", 8), ("f64", 4), ("i32", 0)])
def test_inputs_at_odd_element_offsets(dev, kname, vbytes, off):
    udt = BY_NAME[kname][3]
    na, nb = T + 101, T + 7
    rng = np.random.default_rng(700 + vbytes)
    a, b = (rng.integers(0, 900, size=m).astype(udt) << udt(12) for m in (na, nb))
    va = random_bits(UDT[vbytes], na, rng) if vbytes else None
    vb = random_bits(UDT[vbytes], nb, rng) if vbytes else None
    run_setop(dev, kname, a, b, va, vb, orders=ORDERS, grids=(0, 3), off=off)


def test_overlapping_inputs(dev):
    """A = the first `hi` elements of an array, B = its elements from `lo` on, lo < hi: they share [lo, hi)"""
    rng = np.random.default_rng(71)
    n = 2 * T + 9
    arr = sort_bits(rng.integers(0, 700, size=n).astype(np.uint32), "f32", ASC)
    varr = random_bits(np.uint64, n, rng)
    for lo, hi, grid in ((5, n, 0), (T + 3, T + 900, 3), (0, T, 1)):
        a, b, va, vb = arr[:hi], arr[lo:], varr[:hi], varr[lo:]
        c = Case(dev, "f32", arr, arr[:0], varr, varr[:0], {"keys": np.uint32, "vals": np.uint64, "index": np.uint32})
        # the case's outputs hold n elements; those of the real call need hi and hi + n - lo: give it fresh ones
        outs = {}
        try:
            dev.setParam("debug.setop_grid", grid)
            for op in ALL_OPS:
                index, keys, vals, count = setop_oracle(a, b, "f32", op, ASC, va, vb)
                cap = capacity(op, a.size, b.size)
                sent = {"keys": sentinels(np.uint32, cap, 1), "vals": sentinels(np.uint64, cap, 2), "index": sentinels(np.uint32, cap, 3)}
                outs = {k: Guarded(dev, s, guard_bytes=256, seed=40) for k, s in sent.items()}
                work = Guarded(dev, nbytes=scratch_bytes(dev, 2, 8, a.size, b.size), seed=9, fill=0x5a)
                outs["work"] = work
                c.reset()
                rc = c.call(ASC, op, na=hi, b=c.ins["a"].ptr(lo), vb=c.ins["va"].ptr(lo), nb=b.size, ko=outs["keys"].ptr(), vo=outs["vals"].ptr(),
                            xo=outs["index"].ptr(), work=work.ptr(), work_bytes=work.nbytes)
                assert rc == 0, lib_err()
                s = int(c.count.read(np.uint32)[0])
                assert s == count
                for k, e in (("keys", keys), ("vals", vals), ("index", index)):
                    g = outs[k].read(sent[k].dtype)
                    assert np.array_equal(g[:s], e) and np.array_equal(g[s:], sent[k][s:]), (OPS[op], k, lo, hi)
                work.check_guard()
                c.inputs_unchanged()
                for g in outs.values():
                    g.release()
                outs = {}
        finally:
            dev.setParam("debug.setop_grid", 0)
            for g in outs.values():
                g.release()
            c.release()


# ---------------------------------------------------------------------------------------------
# the work buffer, refusals, empty input
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    rng = np.random.default_rng(81)
    na, nb = 2 * T + 9, T + 1
    a, b = (rng.integers(0, 1500, size=m).astype(np.uint64) for m in (na, nb))
    for fill in (0x00, 0xff, 0x5a):
        run_setop(dev, "f64", a, b, form=("keys", "index"), grids=(0, 3), fill=fill)


def test_scratch_bytes_follow_the_formula(dev):
    chunks = (4 * 8 * int(dev.info.compute_units) + 255) // 256 * 256
    for na, nb in ((0, 0), (1, 0), (T, 0), (T, 1), (1000, 5 * T), (63 * T, 0), (63 * T, 1), (1 << 31, 0xFFF00000 - (1 << 31))):   # (the last: na + nb at the limit)
        tiles = (na + nb + T - 1) // T
        want = chunks + (4 * (tiles + 1) + 255) // 256 * 256
        for kt, vb in ((0, 0), (5, 8), (2, 4)):
            assert scratch_bytes(dev, kt, vb, na, nb) == want, (na, nb)
    sz = ctypes.c_size_t()
    lib = _lib.load()
    for args in ((0, 0, 1 << 31, 0xFFF00001 - (1 << 31)), (0, 0, 0xFFF00001, 0), (0, 0, 1 << 31, 1 << 31), (0, 0, 1 << 32, 0), (0, 0, 0, 1 << 40), (6, 0, 5, 5), (-1, 0, 5, 5), (0, 2, 5, 5), (0, 16, 5, 5)):
        assert lib.adlhip_set_op_scratch_bytes(dev._h, *args, ctypes.byref(sz)) == 1, args
        assert lib_err()


def test_refusals_enqueue_nothing(dev):
    rng = np.random.default_rng(91)
    na, nb = 3000, 2000
    a, b = sort_bits(rng.integers(0, 2500, size=na).astype(np.uint32), "u32", ASC), sort_bits(rng.integers(0, 2500, size=nb).astype(np.uint32), "u32", ASC)
    va, vb = random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng)
    c = Case(dev, "u32", a, b, va, vb, {"keys": np.uint32, "vals": np.uint64, "index": np.uint32})
    wb = c.work.nbytes
    null = ctypes.c_void_p(0)
    U = UNION

    def refused(what, *names, **over):
        rc = c.call(over.pop("order", ASC), over.pop("op", U), **over)
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        for name in names:
            assert name in msg, (what, msg)
        return msg

    try:
        for bad in (-1, 4, 99):
            refused("op %d" % bad, "op", op=bad)
        refused("NULL keys of A", "d_keys_a", a=null)
        refused("NULL keys of B", "d_keys_b", b=null)
        refused("NULL values of A", "d_vals_a", va=null)
        refused("NULL values of B", "d_vals_b", vb=null)
        refused("NULL values out with value_bytes 8", "d_vals_out", vo=null)
        refused("NULL count word", "d_num_out", num=null)
        refused("NULL work", "d_work", work=null)
        refused("no output at all", "d_keys_out", value_bytes=0, va=null, vb=null, ko=null, vo=null, xo=null)
        refused("value_bytes 0 with value arrays", "value_bytes", value_bytes=0)
        refused("value_bytes 0 with one value array", "value_bytes", value_bytes=0, va=null, vb=null)
        for bad in (-1, 2, 16):
            refused("value_bytes %d" % bad, "value_bytes", value_bytes=bad)
        for bad in (-1, 6, 99):
            refused("key_type %d" % bad, "key_type", key_type=bad)
        for bad in (-1, 2):
            refused("order %d" % bad, "order", order=bad)
        refused("misaligned keys of A", "d_keys_a", a=ctypes.c_void_p(c.inp("a").value + 2))
        refused("misaligned keys of B", "d_keys_b", b=ctypes.c_void_p(c.inp("b").value + 1))
        refused("misaligned values of A", "d_vals_a", va=ctypes.c_void_p(c.inp("va").value + 4))
        refused("misaligned values of B", "d_vals_b", vb=ctypes.c_void_p(c.inp("vb").value + 4))
        refused("misaligned keys out", "d_keys_out", ko=c.dout[(True, "keys")].ptr(4), na=na - 1)
        refused("misaligned values out", "d_vals_out", vo=c.dout[(True, "vals")].ptr(8), na=na - 1)
        refused("misaligned index out", "d_index_out", xo=c.dout[(True, "index")].ptr(8), na=na - 2)
        refused("misaligned count word", "d_num_out", num=c.count.ptr(2))
        refused("misaligned work", "d_work", work=c.work.ptr(4), work_bytes=wb - 4)
        refused("keys out is keys of A", "d_keys_out", "d_keys_a", ko=c.inp("a"), nb=0)
        refused("keys out overlaps the end of B", "d_keys_out", "d_keys_b", ko=c.ins["b"].ptr(nb - 4), na=4, nb=nb)
        refused("values out overlaps values of A", "d_vals_out", "d_vals_a", vo=c.ins["va"].ptr(16), na=na - 16, nb=0)
        refused("index out overlaps values of B", "d_index_out", "d_vals_b", xo=c.ins["vb"].ptr(16), na=16, nb=nb)
        refused("index out overlaps keys out", "d_index_out", "d_keys_out", xo=c.dout[(True, "keys")].ptr(16), na=na - 4)
        refused("the count word lies in the keys of B", "d_num_out", "d_keys_b", num=c.ins["b"].ptr(8))
        refused("the count word lies in the index output", "d_index_out", "d_num_out", num=c.dout[(True, "index")].ptr(64))
        refused("the work buffer lies in the keys of A", "d_work", "d_keys_a", work=c.inp("a"))
        refused("na + nb = 2^32", "na + nb", na=(1 << 32) - nb)
        refused("na + nb = 2^32", "na + nb", na=1 << 31, nb=1 << 31)
        refused("na beyond size_t's half", "na + nb", na=(1 << 64) - 1, nb=2)
        msg = refused("work one byte short", "adlhip_set_op_scratch_bytes", work_bytes=wb - 1)
        assert str(wb) in msg
        c.untouched()
        assert dev.getParam("debug.idle_dirty") == 0
        # the proper calls go through
        for op in ALL_OPS:
            c.reset()
            assert c.call(ASC, op) == 0, lib_err()
            index, keys, vals, count = setop_oracle(a, b, "u32", op, ASC, va, vb)
            c.check(op, {"keys": keys, "vals": vals, "index": index}, count, "after the refusals")
    finally:
        c.release()


def test_empty_inputs_clear_the_count_word_only(dev):
    a = np.arange(10, dtype=np.uint32)
    c = Case(dev, "u32", a, a, None, None, {"keys": np.uint32, "index": np.uint32})
    try:
        for op in ALL_OPS:
            c.reset()
            assert c.call(ASC, op, na=0, nb=0) == 0, lib_err()
            c.check(op, {"keys": a[:0], "index": a[:0]}, 0, "empty")
            c.reset()
            assert c.call(DESC, op, na=0, nb=0, a=None, b=None, work=None, work_bytes=0) == 0, lib_err()
            c.check(op, {"keys": a[:0], "index": a[:0]}, 0, "empty, no arrays")
        # refusals come first even then
        c.reset()
        assert c.call(ASC, UNION, na=0, nb=0, ko=None, xo=None) == 1
        assert c.call(ASC, UNION, na=0, nb=0, key_type=7) == 1
        assert c.call(ASC, 4, na=0, nb=0) == 1
        assert c.call(ASC, UNION, na=0, nb=0, num=None) == 1
        c.untouched()
        # one side empty: cap = 0 for an intersection with an empty A
        c.reset()
        assert c.call(ASC, INTERSECTION, na=0) == 0, lib_err()
        c.check(INTERSECTION, {"keys": a[:0], "index": a[:0]}, 0, "empty A")
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        c.release()


# ---------------------------------------------------------------------------------------------
# inputs that are not sorted
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("na,nb", [(T + 1, 3 * T + 5), (3 * T + 7, 3)], ids=lambda v: str(v))
def test_unsorted_inputs_stay_inside_every_buffer(dev, na, nb, grid):
    """The result is unspecified; the call succeeds, the stream reports no fault, the count is at most the capacity, nothing is
    written at the capacity or beyond, every guard is intact and the inputs are unchanged.  (setop_kernels.hpp, BOUNDS: every search
    result lies in its search range whatever the comparisons answer, every look at the other input is compared with its length
    first, and the emit kernel clamps its writes and the count.)  A valid call on valid buffers: this asserts memory safety."""
    rng = np.random.default_rng(900 + na + grid)
    for kname, vbytes, span in (("f32", 8, 1 << 32), ("i64", 4, 50)):
        udt = BY_NAME[kname][3]
        a, b = (rng.integers(0, span, size=m).astype(udt) for m in (na, nb))
        va, vb = random_bits(UDT[vbytes], na, rng), random_bits(UDT[vbytes], nb, rng)
        c = Case(dev, kname, a, b, va, vb, {"keys": udt, "vals": UDT[vbytes], "index": np.uint32})
        dev.setParam("debug.setop_grid", grid)
        try:
            for order in ORDERS:
                for op in ALL_OPS:
                    c.reset()
                    assert c.call(order, op) == 0, lib_err()
                    DeviceUtils.waitForCompletion(dev)        # adlhip_sync: raises on a device fault
                    s, got = c.read()                           # checks the guard behind every output and behind the work buffer
                    assert s <= capacity(op, na, nb)
                    c.count.check_guard()
                    mine = op in (UNION, SYMMETRIC_DIFFERENCE)
                    for (both, k), g in got.items():
                        if both != mine:
                            assert np.array_equal(g, c.sent[(both, k)])
                    c.inputs_unchanged()
                    assert dev.getParam("debug.idle_dirty") == 0
        finally:
            dev.setParam("debug.setop_grid", 0)
            c.release()


# ---------------------------------------------------------------------------------------------
# call sequences, the Pprims mirror
# ---------------------------------------------------------------------------------------------
def test_two_different_operations_back_to_back_through_one_work_buffer(dev):
    rng = np.random.default_rng(55)
    a1, b1 = (sort_bits(rng.integers(0, 2000, size=m).astype(np.uint64), "f64", DESC) for m in (3 * T + 1, T))
    a2, b2 = (sort_bits(rng.integers(0, 300, size=m).astype(np.uint32), "i32", ASC) for m in (T + 9, 7))
    x = Case(dev, "f64", a1, b1, None, None, {"keys": np.uint64, "index": np.uint32})
    y = Case(dev, "i32", a2, b2, None, None, {"keys": np.uint32, "index": np.uint32})
    try:
        for seq in ((0, 1), (1, 0)):
            x.reset()
            y.reset()
            for which in seq:
                rc = x.call(DESC, SYMMETRIC_DIFFERENCE) if which == 0 else y.call(ASC, INTERSECTION, work=x.work.ptr(), work_bytes=x.work.nbytes)
                assert rc == 0, lib_err()
            index, keys, _, count = setop_oracle(a1, b1, "f64", SYMMETRIC_DIFFERENCE, DESC)
            x.check(SYMMETRIC_DIFFERENCE, {"keys": keys, "index": index}, count, "back to back: large")
            index, keys, _, count = setop_oracle(a2, b2, "i32", INTERSECTION, ASC)
            y.check(INTERSECTION, {"keys": keys, "index": index}, count, "back to back: small")
    finally:
        x.release()
        y.release()


def test_pprims_mirror(dev):
    p = Pprims()
    na, nb = T + 11, T // 2 + 1
    rng = np.random.default_rng(66)
    bufs = []

    def dbuf(arr):
        buf = Buffer(dev, max(arr.size, 1), arr.dtype)
        if arr.size:
            buf.write(arr)
        bufs.append(buf)
        return buf

    try:
        for kname, vdt, descending in (("f32", np.int64, False), ("i64", np.float32, True)):
            order = DESC if descending else ASC
            udt, kdt = BY_NAME[kname][3], BY_NAME[kname][2]
            a, b = (sort_bits(rng.integers(0, 700, size=m).astype(udt) << udt(20), kname, order) for m in (na, nb))
            vudt = UDT[np.dtype(vdt).itemsize]
            va, vb = random_bits(vudt, na, rng), random_bits(vudt, nb, rng)
            ba, bb, bva, bvb = dbuf(a.view(kdt)), dbuf(b.view(kdt)), dbuf(va.view(vdt)), dbuf(vb.view(vdt))
            for name in OPS:
                op = OPS.index(name)
                index, keys, vals, count = setop_oracle(a, b, kname, op, order, va, vb)
                cap = capacity(op, na, nb)
                out, vout = Buffer(dev, cap, kdt), Buffer(dev, cap, vdt)
                bufs.extend([out, vout])
                r = p.setOp(dev, name, ba, bb, out, na, nb, descending=descending, valuesA=bva, valuesB=bvb, valuesOut=vout, indexOut=True)
                bufs.extend([r.index, r.count])
                assert r.keys is out and r.values is vout
                assert int(r.count.toHost()[0]) == count
                assert np.array_equal(out.toHost().view(udt)[:count], keys) and np.array_equal(vout.toHost().view(vudt)[:count], vals)
                assert np.array_equal(r.index.toHost()[:count], index)
                mine, cnt = Buffer(dev, cap, np.uint32), Buffer(dev, 1, np.uint32)
                bufs.extend([mine, cnt])
                r = p.setOp(dev, name, ba, bb, None, na, nb, descending=descending, indexOut=mine, countOut=cnt)
                assert r.keys is None and r.values is None and r.index is mine and r.count is cnt
                assert int(cnt.toHost()[0]) == count and np.array_equal(mine.toHost()[:count], index)
            assert np.array_equal(ba.toHost().view(udt), a) and np.array_equal(bb.toHost().view(udt), b)
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for buf in bufs:
            buf.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# the torch front end
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


METHODS = {INTERSECTION: "intersect", UNION: "union", DIFFERENCE: "difference", SYMMETRIC_DIFFERENCE: "symmetric_difference"}
_TORCH_KNAME = {"int32": "i32", "int64": "i64", "float32": "f32", "float64": "f64"}


def _torch_values(dtype, n, seed, span=40):
    """no NaN, no -0 (no zero at all among the floats)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-span, span, (n,), dtype=torch.int64, device="cuda", generator=g)
    if dtype.is_floating_point:
        return torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25
    return t.to(dtype)


def _bits(t):
    x = t.cpu().numpy()
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_set_operations_match_the_oracle(sorter, dtype_name, descending):
    dt = getattr(torch, dtype_name)
    kname = _TORCH_KNAME[dtype_name]
    order = DESC if descending else ASC
    for na, nb, span in ((T + 7, T // 2 + 1, 300), (5, 0, 3), (0, 4, 3), (1, 1, 1), (0, 0, 1)):
        a = torch.sort(_torch_values(dt, na, 21 + na, span), descending=descending, stable=True).values
        b = torch.sort(_torch_values(dt, nb, 22 + nb, span), descending=descending, stable=True).values
        va = _torch_values(torch.int64 if dt != torch.int64 else torch.float32, na, 23, 1000)
        vb = _torch_values(va.dtype, nb, 24, 1000)
        keep = [x.clone() for x in (a, b, va, vb)]
        for op, method in METHODS.items():
            index, keys, vals, count = setop_oracle(_bits(a), _bits(b), kname, op, order, _bits(va), _bits(vb))
            f = getattr(sorter, method)
            got = f(a, b, descending=descending)
            assert isinstance(got, torch.Tensor) and got.dtype == dt and got.numel() == count and np.array_equal(_bits(got), keys)
            k, v, i = f(a, b, descending=descending, values=(va, vb), return_indices=True)
            assert np.array_equal(_bits(k), keys) and i.dtype == torch.int64 and np.array_equal(i.cpu().numpy(), index.astype(np.int64))
            assert v.dtype == va.dtype and np.array_equal(_bits(v), vals)
            k, i = f(a, b, descending=descending, return_indices=True)
            assert np.array_equal(_bits(k), keys) and np.array_equal(i.cpu().numpy(), index.astype(np.int64))
        for x, y in zip((a, b, va, vb), keep):
            assert torch.equal(x, y), "an input was changed"


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_torch_sorter_set_operations_match_numpy_on_duplicate_free_inputs(sorter, dtype_name):
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(12)
    pool = rng.permutation(np.arange(-3000, 3000))
    x, y = np.sort(pool[:T + 300]), np.sort(pool[T:2 * T + 900])          # 300 shared
    a, b = torch.tensor(x, dtype=dt, device="cuda"), torch.tensor(y, dtype=dt, device="cuda")
    want = {"intersect": np.intersect1d(x, y, assume_unique=True), "union": np.union1d(x, y),
            "difference": np.setdiff1d(x, y, assume_unique=True), "symmetric_difference": np.setxor1d(x, y, assume_unique=True)}
    assert want["intersect"].size == 300
    for method, w in want.items():
        got = getattr(sorter, method)(a, b)
        assert got.dtype == dt and np.array_equal(got.cpu().numpy(), w), method
        got = getattr(sorter, method)(a.flip(0), b.flip(0), descending=True)
        assert np.array_equal(got.cpu().numpy(), w[::-1]), method


def test_torch_sorter_set_operations_on_offset_views_make_no_copy(sorter, monkeypatch):
    t = torch.sort(_torch_values(torch.float32, T + 2, 31, 200)).values
    u = torch.sort(_torch_values(torch.int64, T + 4, 32, 200)).values
    seen = []
    real = sorter.pprims.setOp
    monkeypatch.setattr(sorter.pprims, "setOp", lambda dev, op, a, b, *r, **k: (seen.append((a.m_ptr, b.m_ptr)), real(dev, op, a, b, *r, **k))[1])
    for x, y, kname in ((t[1:], t[3:T], "f32"), (u[1:], u[T // 2 + 1:], "i64")):
        assert x.data_ptr() % 16 and y.data_ptr() % 16
        for op, method in METHODS.items():
            index, keys, _, count = setop_oracle(_bits(x), _bits(y), kname, op, ASC)
            got, idx = getattr(sorter, method)(x, y, return_indices=True)
            assert np.array_equal(_bits(got), keys) and np.array_equal(idx.cpu().numpy(), index.astype(np.int64))
            assert seen[-1] == (x.data_ptr(), y.data_ptr()), "a view was copied"
    got = sorter.union(t[::2], t[1::2])                      # strided views are copied, and combined all the same
    assert np.array_equal(_bits(got), setop_oracle(_bits(t[::2]), _bits(t[1::2]), "f32", UNION, ASC)[1])


def test_torch_sorter_set_operations_refuse_what_they_cannot_take(sorter):
    a = torch.arange(6, dtype=torch.int32, device="cuda")
    for method in METHODS.values():
        f = getattr(sorter, method)
        with pytest.raises(TypeError):
            f(a, a.to(torch.int64))
        with pytest.raises(TypeError):
            f(a.to(torch.float16), a.to(torch.float16))
        with pytest.raises(TypeError):
            f(a, [1, 2])
        with pytest.raises(ValueError):
            f(a.reshape(2, 3), a)
        with pytest.raises(ValueError):
            f(a, a, values=(a,))
        with pytest.raises(ValueError):
            f(a, a, values=(a, a[:5]))
        with pytest.raises(TypeError):
            f(a, a, values=(a, a.to(torch.int64)))
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        with pytest.raises(RuntimeError):
            sorter.union(a, a)
    assert sorter.union(a, a[2:]).tolist() == [0, 1, 2, 3, 4, 5]
    assert sorter.intersect(a, a[2:]).tolist() == [2, 3, 4, 5]
    assert sorter.difference(a, a[2:]).tolist() == [0, 1]
    assert sorter.symmetric_difference(a[:4], a[2:]).tolist() == [0, 1, 4, 5]


def test_setop_demo_device_path_matches_its_host_path():
    demo = os.path.join(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), "tests", "demo", "setop_demo")

    def lines(args):
        r = subprocess.run([demo] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.strip()]

    device, host = lines(["--dump"]), lines(["--host", "--dump"])
    assert len(device) == len(host) and len([ln for ln in device if ln.startswith("DUMP ")]) == 3 * 4 * 2 * 2 * 6
    assert all(ln.startswith("[ OK ] SetOp.") for ln in device if ln.startswith("["))
    assert device == host
