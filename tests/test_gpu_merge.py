"""Merge of sorted sequences on the GPU (include/adlhip.h "merge of sorted sequences"; oclradixsort_amd/csrc/merge_kernels.hpp;
Pprims.mergeKeys / mergePairs; TorchSorter.merge).

The oracle is tests/merge_oracle.py (numpy: a stable argsort of the codes of A || B; tests/test_merge_api.py checks it against a
two-pointer loop on the CPU).  Every case is compared bit for bit.

Every output is sized exactly na + nb, prefilled with sentinels and read back whole.  Every device buffer carries guard bytes behind
its payload -- keys, values, every output and the work buffer (sized exactly the reported bytes and prefilled with junk) -- and the
inputs are compared with their originals afterwards.  The handle's device state is idle after each case.

T is the tile of the merge: 2048 output elements.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from merge_oracle import ASC, BY_NAME, DESC, SPECIALS, TYPE_IDS, codes, is_sorted, merge_oracle, sort_bits
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from test_gpu_reduce import Guarded, lib_err, random_bits, sentinels

pytestmark = pytest.mark.gpu

T = 2048
SIZES = [(0, 5), (5, 0), (1, 1), (T - 1, 1), (1, T - 1), (T, T), (T + 1, T - 1), (3, 5 * T + 7), (5 * T + 7, 3), (20 * T + 3, 20 * T + 5)]
GRIDS = [0, 1, 3]
ORDERS = [ASC, DESC]
SENTINELS = 64
UDT = {0: None, 4: np.uint32, 8: np.uint64}
FORMS = [("keys",), ("index",), ("keys", "vals4"), ("keys", "vals8", "index")]


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.merge_grid", 0)
    DeviceUtils.deallocate(d)


def scratch_bytes(dev, key_type, value_bytes, na, nb):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_merge_scratch_bytes(dev._h, key_type, value_bytes, na, nb, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Padded:
    """an input array on the device that starts `off` elements behind a 16-byte boundary, guard bytes behind it"""

    def __init__(self, dev, arr, off, seed):
        self.arr, self.off = arr, off
        self.pad = sentinels(arr.dtype, off, 0x1234 + seed)
        self.g = Guarded(dev, np.concatenate([self.pad, arr]), guard_bytes=SENTINELS * arr.dtype.itemsize, seed=seed)

    def ptr(self, elems=0):
        return self.g.ptr((self.off + elems) * self.arr.dtype.itemsize)

    def unchanged(self):
        return np.array_equal(self.g.read(self.arr.dtype), np.concatenate([self.pad, self.arr]))

    def release(self):
        self.g.release()


class Case:
    """the device side of a series of merges of the same inputs: guarded inputs, sentinel-filled outputs sized exactly na + nb, a work
    buffer of exactly the reported bytes, prefilled with junk.  outs: {name: dtype}"""

    def __init__(self, dev, kname, a, b, va=None, vb=None, outs=None, off=(0, 0), fill=0xff):
        self.dev, self.kname, self.a, self.b, self.va, self.vb = dev, kname, a, b, va, vb
        self.na, self.nb, self.n = a.size, b.size, a.size + b.size
        self.vbytes = va.dtype.itemsize if va is not None else 0
        self.ins = {"a": Padded(dev, a, off[0], 5), "b": Padded(dev, b, off[1], 6)}
        if va is not None:
            self.ins["va"] = Padded(dev, va, off[0], 7)
            self.ins["vb"] = Padded(dev, vb, off[1], 8)
        self.sent = {k: sentinels(dt, self.n, 0xa5a5a5a5a5a5a5a5 + 77 * i) for i, (k, dt) in enumerate(outs.items())}
        self.dout = {k: Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=20 + i) for i, (k, s) in enumerate(self.sent.items())}
        self.work = Guarded(dev, nbytes=scratch_bytes(dev, BY_NAME[kname][1], self.vbytes, self.na, self.nb), seed=9, fill=fill)

    def reset(self):
        for k, s in self.sent.items():
            self.dout[k].buf.write(s.view(np.uint8))

    def inp(self, name):
        return self.ins[name].ptr() if name in self.ins else None

    def out(self, name):
        return self.dout[name].ptr() if name in self.dout else None

    def call(self, order, **over):
        """adlhip_merge_typed on the case's buffers; over: arguments that replace them"""
        arg = dict(key_type=BY_NAME[self.kname][1], order=order, a=self.inp("a"), va=self.inp("va"), na=self.na, b=self.inp("b"),
                   vb=self.inp("vb"), nb=self.nb, value_bytes=self.vbytes, ko=self.out("keys"), vo=self.out("vals"), xo=self.out("index"),
                   work=self.work.ptr(), work_bytes=self.work.nbytes)
        arg.update(over)
        return _lib.load().adlhip_merge_typed(self.dev._h, arg["key_type"], arg["order"], arg["a"], arg["va"], arg["na"], arg["b"], arg["vb"],
                                              arg["nb"], arg["value_bytes"], arg["ko"], arg["vo"], arg["xo"], arg["work"], arg["work_bytes"])

    def read(self):
        """every output, whole; the guards behind every buffer checked"""
        got = {k: g.read(self.sent[k].dtype) for k, g in self.dout.items()}
        self.work.check_guard()
        return got

    def inputs_unchanged(self):
        for k, p in self.ins.items():
            assert p.unchanged(), "input %s was changed" % k

    def check(self, exp, what):
        got = self.read()
        for k, e in exp.items():
            g = got[k]
            assert e.size == self.n == g.size
            if not np.array_equal(g, e):
                bad = np.flatnonzero(g != e)
                raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                    what, k, bad.size, self.n, bad[0], int(g[bad[0]]), int(e[bad[0]])))
        self.inputs_unchanged()
        assert self.dev.getParam("debug.idle_dirty") == 0
        return got

    def untouched(self):
        for k, g in self.dout.items():
            assert np.array_equal(g.read(self.sent[k].dtype), self.sent[k]), "%s was written" % k
        self.inputs_unchanged()
        self.work.check_guard()

    def release(self):
        for b in list(self.ins.values()) + list(self.dout.values()) + [self.work]:
            b.release()


def run_merge(dev, kname, a, b, va=None, vb=None, form=("keys", "vals", "index"), orders=(ASC,), grids=(0,), off=(0, 0), fill=0xff):
    """adlhip_merge_typed on a and b, each sorted here (stably, values along) in every order asked, for every grid, with every check of
    the memory contract.  Returns {(order, grid): the outputs}"""
    form = tuple(k for k in form if k != "vals" or va is not None)
    res = {}
    for order in orders:
        pa, pb = np.argsort(codes(a, kname, order), kind="stable"), np.argsort(codes(b, kname, order), kind="stable")
        sa, sb = a[pa], b[pb]
        sva, svb = (va[pa], vb[pb]) if va is not None else (None, None)
        assert is_sorted(sa, kname, order) and is_sorted(sb, kname, order)
        odt = {k: {"keys": sa.dtype, "vals": sva.dtype if sva is not None else None, "index": np.uint32}[k] for k in form}
        c = Case(dev, kname, sa, sb, sva, svb, odt, off=off, fill=fill)
        index, keys, vals = merge_oracle(sa, sb, kname, order, sva, svb)
        exp = {k: {"keys": keys, "vals": vals, "index": index}[k] for k in form}
        try:
            for grid in grids:
                dev.setParam("debug.merge_grid", grid)
                c.reset()
                what = "merge %s order %d %s na %d nb %d value_bytes %d grid %d off %s" % (kname, order, "+".join(form), sa.size, sb.size,
                                                                                          c.vbytes, grid, off)
                rc = c.call(order)
                assert rc == 0, what + ": " + lib_err()
                res[(order, grid)] = c.check(exp, what)
        finally:
            dev.setParam("debug.merge_grid", 0)
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
# sizes x grids
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", SIZES, ids=["%d+%d" % s for s in SIZES])
def test_sizes_and_grids(dev, na, nb):
    rng = np.random.default_rng(1000 + na + 3 * nb)
    a, b = random_bits(np.uint32, na, rng), random_bits(np.uint32, nb, rng)
    run_merge(dev, "f32", a, b, random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng), orders=ORDERS, grids=GRIDS)
    a, b = random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng)
    run_merge(dev, "i64", a, b, random_bits(np.uint32, na, rng), random_bits(np.uint32, nb, rng), orders=ORDERS, grids=GRIDS)


def test_more_tiles_than_workgroups_on_the_default_grid(dev):
    na, nb = (1 << 22) + 5, (1 << 22) - 9
    assert (na + nb) // T > 8 * int(dev.info.compute_units)
    rng = np.random.default_rng(23)
    a, b = random_bits(np.uint32, na, rng), random_bits(np.uint32, nb, rng)
    run_merge(dev, "i32", a, b, form=("keys", "index"))


# ---------------------------------------------------------------------------------------------
# key patterns
# ---------------------------------------------------------------------------------------------
def _pattern(name, udt, na, nb, rng):
    """(a, b) as bit patterns of unsigned keys, ascending"""
    if name == "random":
        return random_bits(udt, na, rng), random_bits(udt, nb, rng)
    if name == "all_equal":
        return np.full(na, 0x3f800000, udt), np.full(nb, 0x3f800000, udt)
    if name == "a_below_b":
        return np.sort(rng.integers(0, 1000, size=na).astype(udt)), np.sort(rng.integers(1000, 2000, size=nb).astype(udt))
    if name == "b_below_a":
        return np.sort(rng.integers(1000, 2000, size=na).astype(udt)), np.sort(rng.integers(0, 1000, size=nb).astype(udt))
    if name == "strict_alternation":                # a holds the even numbers, b the odd ones
        return np.arange(na, dtype=udt) * udt(2), np.arange(nb, dtype=udt) * udt(2) + udt(1)
    if name == "three_values":                      # runs of about a third of each input: several tiles long, in both
        return np.sort(rng.integers(0, 3, size=na).astype(udt) * udt(7)), np.sort(rng.integers(0, 3, size=nb).astype(udt) * udt(7))
    raise KeyError(name)


PATTERNS = ["random", "all_equal", "a_below_b", "b_below_a", "strict_alternation", "three_values"]


@pytest.mark.parametrize("kname", ["u32", "u64"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_key_patterns(dev, pattern, kname):
    udt = BY_NAME[kname][3]
    rng = np.random.default_rng(PATTERNS.index(pattern))
    for na, nb in ((6 * T + 3, 7 * T + 5), (T + 1, T - 1), (5, 3)):
        a, b = _pattern(pattern, udt, na, nb, rng)
        va, vb = random_bits(np.uint32, na, rng), random_bits(np.uint32, nb, rng)
        res = run_merge(dev, kname, a, b, va, vb, orders=ORDERS, grids=(0, 3))
        if pattern == "all_equal":
            for got in res.values():
                assert np.array_equal(got["index"], np.arange(na + nb, dtype=np.uint32))
        if pattern == "three_values" and na > 4 * T:
            for x in (a, b):
                assert np.bincount(x.astype(np.int64) // 7).min() > 1.5 * T


# ---------------------------------------------------------------------------------------------
# types, orders, forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["asc", "desc"])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_every_key_type_order_and_form_with_special_patterns(dev, kname, order):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    na, nb = 2 * T + 3, 3 * T + 5
    rng = np.random.default_rng(400 + BY_NAME[kname][1])
    a, b = random_bits(udt, na, rng), random_bits(udt, nb, rng)
    for x in (a, b):                                      # specials that repeat, in both inputs: ties between A and B
        x[rng.integers(0, x.size, size=x.size // 3)] = SPECIALS[w][rng.integers(0, SPECIALS[w].size, size=x.size // 3)]
    for form in FORMS:
        names, vbytes = _form(form)
        va = random_bits(UDT[vbytes], na, rng) if vbytes else None
        vb = random_bits(UDT[vbytes], nb, rng) if vbytes else None
        run_merge(dev, kname, a, b, va, vb, form=names, orders=(order,), grids=(0, 1))


# ---------------------------------------------------------------------------------------------
# alignment and aliasing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [(1, 0), (0, 3), (3, 1)], ids=lambda o: "%d_%d" % o)
@pytest.mark.parametrize("kname,vbytes", [("f32", 8), ("f64", 4), ("i32", 0)])
def test_inputs_at_odd_element_offsets(dev, kname, vbytes, off):
    udt = BY_NAME[kname][3]
    na, nb = 3 * T + 1, 2 * T + 7
    rng = np.random.default_rng(700 + vbytes)
    a, b = random_bits(udt, na, rng), random_bits(udt, nb, rng)
    va = random_bits(UDT[vbytes], na, rng) if vbytes else None
    vb = random_bits(UDT[vbytes], nb, rng) if vbytes else None
    run_merge(dev, kname, a, b, va, vb, orders=ORDERS, grids=(0, 3), off=off)


def test_a_and_b_the_same_array_or_overlapping(dev):
    rng = np.random.default_rng(71)
    n = 4 * T + 9
    a = sort_bits(random_bits(np.uint32, n, rng), "f32", ASC)
    va = random_bits(np.uint64, n, rng)
    c = Case(dev, "f32", a, a[:0], va, va[:0], {"keys": np.uint32, "vals": np.uint64, "index": np.uint32})
    try:
        for lo, grid in ((0, 0), (0, 1), (5, 0), (T + 3, 3)):          # B = A[lo:]
            dev.setParam("debug.merge_grid", grid)
            # A = the first lo elements, B = the rest of the same array: n elements in all, as the outputs hold
            index, keys, vals = merge_oracle(a[:lo], a[lo:], "f32", ASC, va[:lo], va[lo:])
            c.reset()
            rc = c.call(ASC, na=lo, b=c.ins["a"].ptr(lo), vb=c.ins["va"].ptr(lo), nb=n - lo)
            assert rc == 0, lib_err()
            c.check({"keys": keys, "vals": vals, "index": index}, "B = A[%d:]" % lo)
    finally:
        dev.setParam("debug.merge_grid", 0)
        c.release()
    # the same array twice: every element of the first copy in front of its twin
    h = 2 * T + 5
    a = sort_bits(random_bits(np.uint64, h, rng), "i64", DESC)
    c = Case(dev, "i64", a, a, None, None, {"keys": np.uint64, "index": np.uint32})
    try:
        index, keys, _ = merge_oracle(a, a, "i64", DESC)
        rc = c.call(DESC, b=c.inp("a"))
        assert rc == 0, lib_err()
        c.check({"keys": keys, "index": index}, "B is A")
    finally:
        c.release()


# ---------------------------------------------------------------------------------------------
# the work buffer, refusals, empty input
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    rng = np.random.default_rng(81)
    na, nb = 5 * T + 9, 2 * T + 1
    a, b = random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng)
    for fill in (0x00, 0xff, 0x5a):
        run_merge(dev, "f64", a, b, form=("keys", "index"), grids=(0, 3), fill=fill)


def test_scratch_bytes_follow_the_formula(dev):
    for na, nb in ((0, 0), (1, 0), (T, 0), (T, 1), (1000, 5 * T), (63 * T, 0), (63 * T, 1), (1 << 31, 0xFFF00000 - (1 << 31))):   # (the last: na + nb at the limit)
        tiles = (na + nb + T - 1) // T
        want = (4 * (tiles + 1) + 255) // 256 * 256
        for kt, vb in ((0, 0), (5, 8), (2, 4)):
            assert scratch_bytes(dev, kt, vb, na, nb) == want, (na, nb)
    sz = ctypes.c_size_t()
    lib = _lib.load()
    for args in ((0, 0, 1 << 31, 0xFFF00001 - (1 << 31)), (0, 0, 0xFFF00001, 0), (0, 0, 1 << 31, 1 << 31), (0, 0, 1 << 32, 0), (0, 0, 0, 1 << 40), (6, 0, 5, 5), (-1, 0, 5, 5), (0, 2, 5, 5), (0, 16, 5, 5)):
        assert lib.adlhip_merge_scratch_bytes(dev._h, *args, ctypes.byref(sz)) == 1, args
        assert lib_err()


def test_refusals_enqueue_nothing(dev):
    rng = np.random.default_rng(91)
    na, nb = 3000, 2000
    a, b = sort_bits(random_bits(np.uint32, na, rng), "u32", ASC), sort_bits(random_bits(np.uint32, nb, rng), "u32", ASC)
    va, vb = random_bits(np.uint64, na, rng), random_bits(np.uint64, nb, rng)
    c = Case(dev, "u32", a, b, va, vb, {"keys": np.uint32, "vals": np.uint64, "index": np.uint32})
    wb = c.work.nbytes
    null = ctypes.c_void_p(0)

    def refused(what, *names, **over):
        rc = c.call(over.pop("order", ASC), **over)
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        for name in names:
            assert name in msg, (what, msg)
        return msg

    try:
        refused("NULL keys of A", "d_keys_a", a=null)
        refused("NULL keys of B", "d_keys_b", b=null)
        refused("NULL values of A", "d_vals_a", va=null)
        refused("NULL values of B", "d_vals_b", vb=null)
        refused("NULL values out with value_bytes 8", "d_vals_out", vo=null)
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
        refused("misaligned keys out", "d_keys_out", ko=c.dout["keys"].ptr(4), na=na - 1)
        refused("misaligned values out", "d_vals_out", vo=c.dout["vals"].ptr(8), na=na - 1)
        refused("misaligned index out", "d_index_out", xo=c.dout["index"].ptr(8), na=na - 2)
        refused("misaligned work", "d_work", work=c.work.ptr(4), work_bytes=wb - 4)
        refused("keys out is keys of A", "d_keys_out", "d_keys_a", ko=c.inp("a"), nb=0)
        refused("keys out overlaps the end of B", "d_keys_out", "d_keys_b", ko=c.ins["b"].ptr(nb - 4), na=4, nb=nb)
        refused("values out overlaps values of A", "d_vals_out", "d_vals_a", vo=c.ins["va"].ptr(16), na=na - 16, nb=0)
        refused("index out overlaps values of B", "d_index_out", "d_vals_b", xo=c.ins["vb"].ptr(16), na=16, nb=nb)
        refused("index out overlaps keys out", "d_index_out", "d_keys_out", xo=c.dout["keys"].ptr(16), na=na - 4)
        refused("values out overlaps keys out", "d_keys_out", "d_vals_out", vo=c.dout["keys"].ptr(0), na=(na + nb) // 2 - nb)
        refused("the work buffer lies in the keys of A", "d_work", "d_keys_a", work=c.inp("a"))
        refused("na + nb = 2^32", "na + nb", na=(1 << 32) - nb)
        refused("na + nb = 2^32", "na + nb", na=1 << 31, nb=1 << 31)
        refused("na beyond size_t's half", "na + nb", na=(1 << 64) - 1, nb=2)
        msg = refused("work one byte short", "adlhip_merge_scratch_bytes", work_bytes=wb - 1)
        assert str(wb) in msg
        c.untouched()
        assert dev.getParam("debug.idle_dirty") == 0
        # the proper call goes through
        assert c.call(ASC) == 0, lib_err()
        index, keys, vals = merge_oracle(a, b, "u32", ASC, va, vb)
        c.check({"keys": keys, "vals": vals, "index": index}, "after the refusals")
    finally:
        c.release()


def test_empty_merge_succeeds_and_enqueues_nothing(dev):
    a = np.arange(10, dtype=np.uint32)
    c = Case(dev, "u32", a, a, None, None, {"keys": np.uint32, "index": np.uint32})
    try:
        assert c.call(ASC, na=0, nb=0) == 0, lib_err()
        assert c.call(DESC, na=0, nb=0, a=None, b=None, work=None, work_bytes=0) == 0, lib_err()
        c.untouched()
        # refusals come first even then
        assert c.call(ASC, na=0, nb=0, ko=None, xo=None) == 1
        assert c.call(ASC, na=0, nb=0, key_type=7) == 1
        c.untouched()
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        c.release()


# ---------------------------------------------------------------------------------------------
# inputs that are not sorted
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("na,nb", [(T + 1, 3 * T + 5), (5 * T + 7, 3)], ids=lambda v: str(v))
def test_unsorted_inputs_stay_inside_every_buffer(dev, na, nb, grid):
    """The order of the output is unspecified; the call succeeds, the stream reports no fault, nothing is written outside the na + nb
    elements of the outputs, every guard is intact and the inputs are unchanged.  (merge_kernels.hpp, BOUNDS: every split lies in its
    search range whatever the comparisons answer, and a tile's share of A is clamped to the tile.)"""
    rng = np.random.default_rng(900 + na + grid)
    for kname, vbytes in (("f32", 8), ("i64", 4)):
        udt = BY_NAME[kname][3]
        a, b = random_bits(udt, na, rng), random_bits(udt, nb, rng)
        va, vb = random_bits(UDT[vbytes], na, rng), random_bits(UDT[vbytes], nb, rng)
        c = Case(dev, kname, a, b, va, vb, {"keys": udt, "vals": UDT[vbytes], "index": np.uint32})
        dev.setParam("debug.merge_grid", grid)
        try:
            for order in ORDERS:
                c.reset()
                assert c.call(order) == 0, lib_err()
                DeviceUtils.waitForCompletion(dev)        # adlhip_sync: raises on a device fault
                got = c.read()                              # checks the guard behind every output and behind the work buffer
                c.inputs_unchanged()
                assert dev.getParam("debug.idle_dirty") == 0
                assert all(g.size == na + nb for g in got.values())
        finally:
            dev.setParam("debug.merge_grid", 0)
            c.release()


# ---------------------------------------------------------------------------------------------
# call sequences, the Pprims mirror
# ---------------------------------------------------------------------------------------------
def test_two_different_merges_back_to_back_through_one_work_buffer(dev):
    """nothing is remembered between calls: a large merge, then a small one of another type through the same work buffer, read back
    only after both were enqueued; then the other way round"""
    rng = np.random.default_rng(55)
    a1, b1 = sort_bits(random_bits(np.uint64, 6 * T + 1, rng), "f64", DESC), sort_bits(random_bits(np.uint64, 3 * T, rng), "f64", DESC)
    a2, b2 = sort_bits(random_bits(np.uint32, T + 9, rng), "i32", ASC), sort_bits(random_bits(np.uint32, 7, rng), "i32", ASC)
    x = Case(dev, "f64", a1, b1, None, None, {"keys": np.uint64, "index": np.uint32})
    y = Case(dev, "i32", a2, b2, None, None, {"keys": np.uint32, "index": np.uint32})
    try:
        for seq in ((0, 1), (1, 0)):
            x.reset()
            y.reset()
            for which in seq:
                rc = x.call(DESC) if which == 0 else y.call(ASC, work=x.work.ptr(), work_bytes=x.work.nbytes)
                assert rc == 0, lib_err()
            index, keys, _ = merge_oracle(a1, b1, "f64", DESC)
            x.check({"keys": keys, "index": index}, "back to back: large")
            index, keys, _ = merge_oracle(a2, b2, "i32", ASC)
            y.check({"keys": keys, "index": index}, "back to back: small")
    finally:
        x.release()
        y.release()


def test_pprims_mirror(dev):
    p = Pprims()
    na, nb = 3 * T + 11, 2 * T + 1
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
            a, b = sort_bits(random_bits(udt, na, rng), kname, order), sort_bits(random_bits(udt, nb, rng), kname, order)
            vudt = UDT[np.dtype(vdt).itemsize]
            va, vb = random_bits(vudt, na, rng), random_bits(vudt, nb, rng)
            index, keys, vals = merge_oracle(a, b, kname, order, va, vb)
            ba, bb, bva, bvb = dbuf(a.view(kdt)), dbuf(b.view(kdt)), dbuf(va.view(vdt)), dbuf(vb.view(vdt))
            out, vout = Buffer(dev, na + nb, kdt), Buffer(dev, na + nb, vdt)
            bufs.extend([out, vout])
            idx = p.mergeKeys(dev, ba, bb, out, na, nb, descending=descending, indexOut=True)
            bufs.append(idx)
            assert np.array_equal(out.toHost().view(udt), keys) and np.array_equal(idx.toHost(), index)
            assert p.mergeKeys(dev, ba, bb, out, na, nb, descending=descending) is None
            mine = Buffer(dev, na + nb, np.uint32)
            bufs.append(mine)
            assert p.mergePairs(dev, ba, bva, bb, bvb, None, vout, na, nb, descending=descending, indexOut=mine) is mine
            assert np.array_equal(vout.toHost().view(vudt), vals) and np.array_equal(mine.toHost(), index)
            assert p.mergePairs(dev, ba, bva, bb, bvb, out, vout, 0, nb, descending=descending) is None          # one side empty
            assert np.array_equal(out.toHost().view(udt)[:nb], b) and np.array_equal(vout.toHost().view(vudt)[:nb], vb)
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


def _torch_values(dtype, n, seed, span=40):
    """no NaN, no -0 (no zero at all among the floats)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-span, span, (n,), dtype=torch.int64, device="cuda", generator=g)
    if dtype.is_floating_point:
        return torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25
    return t.to(dtype)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_merge_matches_torch_sort_of_the_concatenation(sorter, dtype_name, descending):
    dt = getattr(torch, dtype_name)
    for na, nb, span in ((3 * T + 7, 2 * T + 1, 40), (5, 0, 3), (0, 4, 3), (1, 1, 1), (0, 0, 1), (T, T, 100000)):
        a = torch.sort(_torch_values(dt, na, 21 + na, span), descending=descending, stable=True).values
        b = torch.sort(_torch_values(dt, nb, 22 + nb, span), descending=descending, stable=True).values
        va = _torch_values(torch.int64 if dt != torch.int64 else torch.float32, na, 23, 1000)
        vb = _torch_values(va.dtype, nb, 24, 1000)
        keep = [x.clone() for x in (a, b, va, vb)]
        want = torch.sort(torch.cat((a, b)), descending=descending, stable=True)
        got = sorter.merge(a, b, descending=descending)
        assert isinstance(got, torch.Tensor) and got.dtype == dt and torch.equal(got, want.values)
        k, v, i = sorter.merge(a, b, descending=descending, values=(va, vb), return_indices=True)
        assert torch.equal(k, want.values) and i.dtype == torch.int64 and torch.equal(i, want.indices)
        assert v.dtype == va.dtype and torch.equal(v, torch.cat((va, vb))[want.indices])
        k, i = sorter.merge(a, b, descending=descending, return_indices=True)
        assert torch.equal(k, want.values) and torch.equal(i, want.indices)
        for x, y in zip((a, b, va, vb), keep):
            assert torch.equal(x, y), "an input was changed"


def test_torch_sorter_merge_of_offset_views_makes_no_copy(sorter, monkeypatch):
    t = torch.sort(_torch_values(torch.float32, 3 * T + 2, 31)).values
    u = torch.sort(_torch_values(torch.int64, 2 * T + 4, 32)).values
    seen = []
    real = sorter.pprims.mergeKeys
    monkeypatch.setattr(sorter.pprims, "mergeKeys", lambda dev, a, b, *r, **k: (seen.append((a.m_ptr, b.m_ptr)), real(dev, a, b, *r, **k))[1])
    for x, y in ((t[1:], t[3:T]), (u[1:], u[T + 1:])):
        assert x.data_ptr() % 16 and y.data_ptr() % 16
        got, idx = sorter.merge(x, y, return_indices=True)
        want = torch.sort(torch.cat((x, y)), stable=True)
        assert torch.equal(got, want.values) and torch.equal(idx, want.indices)
        assert seen[-1] == (x.data_ptr(), y.data_ptr()), "a view was copied"
    got = sorter.merge(t[::2], t[1::2])                      # strided views are copied, and merged all the same
    assert torch.equal(got, torch.sort(torch.cat((t[::2], t[1::2])), stable=True).values)


def test_torch_sorter_merge_refuses_what_it_cannot_merge(sorter):
    a = torch.arange(6, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        sorter.merge(a, a.to(torch.int64))
    with pytest.raises(TypeError):
        sorter.merge(a.to(torch.float16), a.to(torch.float16))
    with pytest.raises(TypeError):
        sorter.merge(a, [1, 2])
    with pytest.raises(ValueError):
        sorter.merge(a.reshape(2, 3), a)
    with pytest.raises(ValueError):
        sorter.merge(a, a, values=(a,))
    with pytest.raises(ValueError):
        sorter.merge(a, a, values=(a, a[:5]))
    with pytest.raises(TypeError):
        sorter.merge(a, a, values=(a, a.to(torch.int64)))
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        with pytest.raises(RuntimeError):
            sorter.merge(a, a)
    assert sorter.merge(a, a).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


def test_merge_demo_device_path_matches_its_host_path():
    demo = os.path.join(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), "tests", "demo", "merge_demo")

    def lines(args):
        r = subprocess.run([demo] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.strip()]

    device, host = lines(["--dump"]), lines(["--host", "--dump"])
    assert len(device) == len(host) and len([ln for ln in device if ln.startswith("DUMP ")]) == 4 * 2 * 3 * 6
    assert all(ln.startswith("[ OK ] Merge.") for ln in device if ln.startswith("["))
    assert device == host
