"""Sorted search on the GPU (include/adlhip.h "sorted search"; oclradixsort_amd/csrc/search_kernels.hpp; Pprims.searchSorted;
TorchSorter.searchsorted / bucketize).

The oracle is tests/search_oracle.py (numpy: np.searchsorted on the codes; tests/test_search_api.py checks it against a counting
loop on the CPU).  Every case is compared exactly.

The output is sized exactly n, prefilled with sentinels and read back whole.  Every device buffer carries guard bytes behind its
payload, and the inputs are compared with their originals afterwards.  The handle's device state is idle after each case.

T is the tile of the search: 2048 needles.  C is the capacity of the table in LDS, read with get_param.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from search_oracle import ASC, BY_NAME, DESC, LEFT, RIGHT, SPECIALS, TYPE_IDS, codes, decode, is_sorted, search_oracle, sort_bits
from test_gpu_merge import Padded
from test_gpu_reduce import Guarded, lib_err, random_bits, sentinels

pytestmark = pytest.mark.gpu

T = 2048
NEEDLE_COUNTS = [0, 1, T - 1, T, T + 1, 5 * T + 7, 20 * T + 3]
GRIDS = [0, 1, 3]
ORDERS = [ASC, DESC]
SIDES = [LEFT, RIGHT]
SENTINELS = 64
KNOBS = ("debug.search_grid", "debug.search_lds_keys")


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    for k in KNOBS:
        d.setParam(k, 0)
    DeviceUtils.deallocate(d)


@pytest.fixture(scope="module")
def C(dev):
    dev.setParam("debug.search_lds_keys", 0)
    c = dev.getParam("debug.search_lds_keys")
    assert c >= 16
    return c


class Case:
    """the device side of a series of searches of the same inputs: the sequence `off` elements behind a 16-byte boundary, the needles
    in a buffer of their own -- or, with alias, the sequence's own buffer from its 16-byte boundary on: the `off` elements in front of
    the sequence and the sequence itself --, the positions sized exactly n and filled with sentinels; guard bytes behind each"""

    def __init__(self, dev, kname, seq, needles=None, off=0, alias=False):
        self.dev, self.kname, self.seq, self.m = dev, kname, seq, seq.size
        self.s = Padded(dev, seq, off, 5)
        if alias:
            self.needles, self.x = np.concatenate([self.s.pad, seq]), None
        else:
            self.needles = needles
            self.x = Guarded(dev, needles, guard_bytes=SENTINELS * needles.dtype.itemsize, seed=6)
        self.n = self.needles.size
        self.sent = sentinels(np.uint32, self.n, 0xa5a5a5a5a5a5a5a5)
        self.pos = Guarded(dev, self.sent, guard_bytes=SENTINELS * 4, seed=20)

    def reset(self):
        if self.n:
            self.pos.buf.write(self.sent.view(np.uint8))

    def needle_ptr(self):
        return self.x.ptr() if self.x is not None else self.s.g.ptr()

    def call(self, order, side, **over):
        """adlhip_search_sorted_typed on the case's buffers; over: arguments that replace them"""
        arg = dict(key_type=BY_NAME[self.kname][1], order=order, side=side, sorted=self.s.ptr(), m=self.m, needles=self.needle_ptr(), n=self.n,
                   pos=self.pos.ptr())
        arg.update(over)
        return _lib.load().adlhip_search_sorted_typed(self.dev._h, arg["key_type"], arg["order"], arg["side"], arg["sorted"], arg["m"],
                                                      arg["needles"], arg["n"], arg["pos"])

    def inputs_unchanged(self):
        assert self.s.unchanged(), "the sequence was changed"
        if self.x is not None:
            assert np.array_equal(self.x.read(self.needles.dtype), self.needles), "the needles were changed"

    def read(self):
        """every position, whole; the guards behind every buffer checked"""
        got = self.pos.read(np.uint32)
        self.inputs_unchanged()
        assert self.dev.getParam("debug.idle_dirty") == 0
        return got

    def check(self, exp, what):
        got = self.read()
        assert exp.size == self.n == got.size
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError("%s: positions differ at %d of %d places, first at %d: got %d, expected %d" % (
                what, bad.size, self.n, bad[0], int(got[bad[0]]), int(exp[bad[0]])))
        return got

    def untouched(self):
        assert np.array_equal(self.pos.read(np.uint32), self.sent), "the positions were written"
        self.inputs_unchanged()

    def release(self):
        for b in (self.s, self.x, self.pos):
            if b is not None:
                b.release()


def run_search(dev, kname, seq, needles=None, orders=(ASC,), sides=SIDES, grids=(0,), tables=(0,), off=0, alias=False):
    """adlhip_search_sorted_typed on seq, sorted here in every order asked, for every side, grid and table capacity, with every check
    of the memory contract.  Returns {(order, side, grid, table): the positions}"""
    res = {}
    for order in orders:
        s = sort_bits(seq, kname, order)
        assert is_sorted(s, kname, order)
        c = Case(dev, kname, s, needles, off=off, alias=alias)
        try:
            for side in sides:
                exp = search_oracle(s, c.needles, kname, order, side)
                for table in tables:
                    for grid in grids:
                        dev.setParam("debug.search_lds_keys", table)
                        dev.setParam("debug.search_grid", grid)
                        c.reset()
                        what = "search %s order %d side %d m %d n %d grid %d table %d off %d" % (kname, order, side, s.size, c.n, grid, table, off)
                        rc = c.call(order, side)
                        assert rc == 0, what + ": " + lib_err()
                        res[(order, side, grid, table)] = c.check(exp, what)
        finally:
            for k in KNOBS:
                dev.setParam(k, 0)
            c.release()
    return res


def needle_set(seq, kname, rng, extra=0):
    """bit patterns, whatever the order: every element of the sequence, every element's ascending code + 1 and - 1 (the neighbours in
    either order), the specials, `extra` random patterns, and as many of the smallest and of the largest code"""
    udt = seq.dtype.type
    w = seq.dtype.itemsize
    c = codes(seq, kname, ASC)
    one, ones = udt(1), ~udt(0)
    parts = [seq, decode(c[c != ones] + one, kname), decode(c[c != 0] - one, kname), SPECIALS[w], random_bits(seq.dtype, extra, rng, specials=False),
             decode(np.zeros(5, seq.dtype), kname), decode(np.full(5, ones, seq.dtype), kname)]
    x = np.concatenate(parts)
    return x[rng.permutation(x.size)]


# ---------------------------------------------------------------------------------------------
# needle counts x grids
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NEEDLE_COUNTS)
def test_needle_counts_and_grids(dev, C, n):
    rng = np.random.default_rng(1000 + n)
    for kname, m, table in (("f32", 1000, 0), ("i64", 5 * 64 + 3, 64)):   # the search that ends in LDS; the two-level one
        udt = BY_NAME[kname][3]
        seq = random_bits(udt, m, rng)
        needles = random_bits(udt, n, rng)
        if n > 4:
            needles[::3] = seq[rng.integers(0, m, size=needles[::3].size)]
        run_search(dev, kname, seq, needles, orders=ORDERS, grids=GRIDS, tables=(table,))


# ---------------------------------------------------------------------------------------------
# sequence lengths around the table
# ---------------------------------------------------------------------------------------------
def test_default_table_lengths(dev, C):
    rng = np.random.default_rng(7)
    for m in (0, 1, 2, C - 1, C, C + 1):
        for kname in ("u32", "f64"):
            seq = random_bits(BY_NAME[kname][3], m, rng)
            needles = needle_set(seq, kname, rng, extra=T + 1)
            res = run_search(dev, kname, seq, needles, orders=ORDERS, grids=(0, 1))
            if m == 0:
                assert all(not got.any() for got in res.values())


def lowered_lengths(table):
    return sorted({k * table + d for k in (1, 2, 63) for d in (-1, 0, 1)} | {100003})


@pytest.mark.parametrize("table", [2, 3, 16])
def test_lowered_table_lengths(dev, C, table):
    """the stride 1 / stride 2 boundary, blocks that are exactly full, a last block of one element, and with 100 003 elements a
    search of 15 steps and more in global memory"""
    assert table <= C
    rng = np.random.default_rng(70 + table)
    for m in lowered_lengths(table):
        if m < 1:
            continue
        stride = -(-m // table)
        if m == 100003:
            assert stride >= 1 << 12
        for kname in ("i32", "u64"):
            seq = random_bits(BY_NAME[kname][3], m, rng)
            needles = needle_set(seq, kname, rng, extra=300)
            if needles.size > 4 * T + 9:
                needles = needles[:4 * T + 9]
            run_search(dev, kname, seq, needles, orders=ORDERS, grids=(0, 3), tables=(table,))


def test_three_mi_elements_on_the_default_table(dev, C):
    m = 3 * (1 << 20) + 5
    rng = np.random.default_rng(99)
    seq = random_bits(np.uint32, m, rng)
    pick = seq[rng.integers(0, m, size=40000)]
    c = codes(pick, "f32", ASC)
    needles = np.concatenate([pick, decode(c + np.uint32(1), "f32"), decode(c - np.uint32(1), "f32"), random_bits(np.uint32, 3 * T + 1, rng),
                              seq[:3], seq[-3:]])
    run_search(dev, "f32", seq, needles, orders=(ASC,))
    run_search(dev, "f32", seq, needles, orders=(DESC,), sides=(RIGHT,))


# ---------------------------------------------------------------------------------------------
# needle and sequence patterns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", ["u32", "u64"])
def test_needles_outside_the_sequence(dev, C, kname):
    udt = BY_NAME[kname][3]
    rng = np.random.default_rng(5)
    for table, m in ((0, 700), (16, 16 * 9 + 5)):
        seq = rng.integers(1000, 2000, size=m).astype(udt)
        below, above = rng.integers(0, 1000, size=T + 3).astype(udt), rng.integers(2000, 3000, size=T + 3).astype(udt)
        for order in ORDERS:
            lo, hi = (0, m) if order == ASC else (m, 0)
            for got in run_search(dev, kname, seq, below, orders=(order,), tables=(table,), grids=(0, 1)).values():
                assert (got == lo).all()
            for got in run_search(dev, kname, seq, above, orders=(order,), tables=(table,), grids=(0, 1)).values():
                assert (got == hi).all()


@pytest.mark.parametrize("kname", ["f32", "i64"])
def test_one_repeated_key_longer_than_several_blocks(dev, C, kname):
    udt = BY_NAME[kname][3]
    key = udt(0x3f800000)
    for table, m in ((16, 16 * 40 + 3), (0, 2 * C + 7), (0, 100)):
        seq = np.full(m, key, udt)
        c = codes(seq[:1], kname, ASC)
        needles = np.concatenate([np.full(T + 5, key, udt), decode(c + udt(1), kname), decode(c - udt(1), kname)])
        res = run_search(dev, kname, seq, needles, orders=ORDERS, tables=(table,), grids=(0, 1))
        for (order, side, _, _), got in res.items():
            assert (got[:T + 5] == (0 if side == LEFT else m)).all()
            assert got[T + 5] == (m if order == ASC else 0) and got[T + 6] == (0 if order == ASC else m)


@pytest.mark.parametrize("kname", ["i32", "f64"])
def test_runs_that_straddle_block_boundaries(dev, C, kname):
    udt = BY_NAME[kname][3]
    rng = np.random.default_rng(11)
    for table, m, values in ((16, 16 * 50 + 9, 5), (3, 1000, 2), (0, 4 * C + 3, 7)):
        stride = -(-m // (table or C))
        seq = (rng.integers(0, values, size=m) * 5).astype(udt)       # few values: every run is longer than a block
        assert np.bincount(seq.astype(np.int64) // 5).min() > stride
        needles = np.concatenate([np.arange(0, 40, dtype=udt), (udt(0) - np.arange(1, 9, dtype=udt)), seq[:T]])
        run_search(dev, kname, seq, needles, orders=ORDERS, tables=(table,), grids=(0, 3))


# ---------------------------------------------------------------------------------------------
# types, orders, sides; views at odd offsets; needles that alias the sequence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["asc", "desc"])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_every_key_type_order_and_side_with_special_patterns(dev, C, kname, order):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    rng = np.random.default_rng(400 + BY_NAME[kname][1])
    for table, m in ((0, T + 3), (16, 16 * 7 + 1)):
        seq = random_bits(udt, m, rng)
        seq[rng.integers(0, m, size=m // 3)] = SPECIALS[w][rng.integers(0, SPECIALS[w].size, size=m // 3)]   # specials that repeat
        needles = needle_set(seq, kname, rng, extra=100)
        for off in (0, 1, 3):
            run_search(dev, kname, seq, needles, orders=(order,), tables=(table,), off=off)
            run_search(dev, kname, seq, orders=(order,), tables=(table,), off=off, alias=True)   # needles = the sequence's own buffer


# ---------------------------------------------------------------------------------------------
# a sequence that is not sorted
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", ["u32", "f64"])
def test_an_unsorted_sequence_stays_inside_the_arrays(dev, C, kname):
    udt = BY_NAME[kname][3]
    rng = np.random.default_rng(77)
    try:
        for m, n in ((1, 5), (C - 1, 3 * T + 1), (C + 1, T), (5 * C + 3, 2 * T + 9), (100003, T + 1)):
            seq = random_bits(udt, m, rng)
            if m > 2:
                assert not is_sorted(seq, kname, ASC)
            c = Case(dev, kname, seq, random_bits(udt, n, rng), off=1)
            try:
                for table in (0, 2, 3, 16):
                    for grid in (0, 1, 3):
                        for side in SIDES:
                            dev.setParam("debug.search_lds_keys", table)
                            dev.setParam("debug.search_grid", grid)
                            c.reset()
                            assert c.call(ASC, side) == 0, lib_err()
                            got = c.read()          # the guards and the inputs are checked here
                            assert (got <= m).all(), (m, n, table, grid, side)
            finally:
                c.release()
    finally:
        for k in KNOBS:
            dev.setParam(k, 0)


# ---------------------------------------------------------------------------------------------
# what is already merged
# ---------------------------------------------------------------------------------------------
def _search(dev, p, kdt, seq_buf, m, needles_buf, n, order, side):
    pos = Buffer(dev, max(n, 1), np.uint32)
    p.searchSorted(dev, seq_buf, needles_buf, pos, m, n, descending=order == DESC, right=side == RIGHT)
    got = pos.toHost()[:n]
    pos.release()
    return got


@pytest.mark.parametrize("kname", ["f32", "i64"])
def test_the_merge_puts_a_at_i_plus_left_b_and_b_at_j_plus_right_a(dev, C, kname):
    udt, kdt = BY_NAME[kname][3], BY_NAME[kname][2]
    rng = np.random.default_rng(3)
    p = Pprims()
    try:
        for order in ORDERS:
            na, nb = 3 * T + 5, 2 * T + 1
            a = sort_bits((rng.integers(0, 500, size=na) * 3).astype(udt), kname, order)      # many ties between A and B
            b = sort_bits((rng.integers(0, 500, size=nb) * 3).astype(udt), kname, order)
            A, B, out = Buffer(dev, na, kdt), Buffer(dev, nb, kdt), Buffer(dev, na + nb, kdt)
            A.write(a.view(kdt))
            B.write(b.view(kdt))
            idx = p.mergeKeys(dev, A, B, out, na, nb, descending=order == DESC, indexOut=True)
            index = idx.toHost()
            left_b = _search(dev, p, kdt, B, nb, A, na, order, LEFT)
            right_a = _search(dev, p, kdt, A, na, B, nb, order, RIGHT)
            where = np.empty(na + nb, np.int64)              # where[e] = the output position of element e of A || B
            where[index] = np.arange(na + nb)
            assert np.array_equal(where[:na], np.arange(na) + left_b)
            assert np.array_equal(where[na:], np.arange(nb) + right_a)
            for buf in (A, B, out, idx):
                buf.release()
    finally:
        p.close()
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("kname", ["i32", "f32", "u64"])
def test_bincount_of_right_minus_one_is_the_range_histogram(dev, C, kname):
    udt, kdt = BY_NAME[kname][3], BY_NAME[kname][2]
    rng = np.random.default_rng(13)
    p = Pprims()
    try:
        for bins in (1, 255, 4096):
            n = 5 * T + 3
            keys = random_bits(udt, n, rng)
            edges = sort_bits(random_bits(udt, 3 * (bins + 1), rng, specials=False), kname)
            edges = edges[np.concatenate([[True], codes(edges, kname)[1:] != codes(edges, kname)[:-1]])][:bins + 1]   # strictly increasing
            assert edges.size == bins + 1
            keys[::5] = edges[rng.integers(0, bins + 1, size=keys[::5].size)]      # keys on the edges, the last one included
            K, E = Buffer(dev, n, kdt), Buffer(dev, bins + 1, kdt)
            K.write(keys.view(kdt))
            E.write(edges.view(kdt))
            counts = p.histogramRange(dev, K, n, E, bins)
            want = counts.toHost()[:bins]
            pos = _search(dev, p, kdt, E, bins + 1, K, n, ASC, RIGHT).astype(np.int64) - 1
            inside = (pos >= 0) & (pos < bins)
            assert np.array_equal(np.bincount(pos[inside], minlength=bins).astype(np.uint32), want)
            for buf in (K, E, counts):
                buf.release()
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_every_refusal_names_its_argument_and_enqueues_nothing(dev, C):
    rng = np.random.default_rng(1)
    m, n = 300, 200
    c = Case(dev, "f32", sort_bits(random_bits(np.uint32, m, rng), "f32"), random_bits(np.uint32, n, rng))
    c8 = Case(dev, "i64", sort_bits(random_bits(np.uint64, m, rng), "i64"), random_bits(np.uint64, n, rng))

    def off(ptr, nbytes):
        return ctypes.c_void_p(ptr.value + nbytes)
    try:
        c.reset()
        c8.reset()
        cases = [
            (c, dict(sorted=None), "d_sorted is required"),
            (c, dict(needles=None), "d_needles is required"),
            (c, dict(pos=None), "d_pos_out is required"),
            (c, dict(sorted=off(c.s.ptr(), 2)), "d_sorted must be 4-byte aligned"),
            (c8, dict(sorted=off(c8.s.ptr(), 4)), "d_sorted must be 8-byte aligned"),
            (c, dict(needles=off(c.needle_ptr(), 4), n=n - 1), "d_needles must be 16-byte aligned"),
            (c8, dict(needles=off(c8.needle_ptr(), 8), n=n - 1), "d_needles must be 16-byte aligned"),
            (c, dict(pos=off(c.pos.ptr(), 4), n=n - 1), "d_pos_out must be 16-byte aligned"),
            (c, dict(pos=c.needle_ptr()), "d_pos_out must not overlap d_needles"),
            (c, dict(pos=off(c.needle_ptr(), 4 * n - 16)), "d_pos_out must not overlap d_needles"),
            (c, dict(pos=c.s.ptr()), "d_pos_out must not overlap d_sorted"),
            (c, dict(needles=c.pos.ptr()), "d_pos_out must not overlap d_needles"),
            (c, dict(key_type=6), "key_type"),
            (c, dict(key_type=-1), "key_type"),
            (c, dict(order=2), "order must be"),
            (c, dict(order=-1), "order must be"),
            (c, dict(side=2), "side must be ADLHIP_SEARCH_LEFT (0) or ADLHIP_SEARCH_RIGHT (1), got 2"),
            (c, dict(side=-1), "side must be"),
            (c, dict(m=1 << 32), "m = 4294967296 exceeds"),
            (c, dict(n=1 << 32), "n = 4294967296 exceeds"),
            (c8, dict(m=(1 << 32) + 5), "m = 4294967301 exceeds"),
        ]
        for case, over, text in cases:
            rc = case.call(**{"order": ASC, "side": LEFT, **over})
            assert rc == 1, (over, text)
            assert text in lib_err(), (over, lib_err())
            assert "search sorted" in lib_err() or "key_type" in text or "order" in text, lib_err()
        c.untouched()
        c8.untouched()
        # m == 0: the sequence is not looked at, n zeros are written; n == 0: nothing is
        assert c.call(ASC, RIGHT, sorted=None, m=0) == 0, lib_err()
        assert not c.read().any()
        c.reset()
        assert c.call(ASC, RIGHT, n=0, needles=None, pos=None) == 0, lib_err()
        c.untouched()
        # the same array as sequence and needles
        s = c.seq
        assert n < m
        assert c.call(ASC, LEFT, needles=c.s.ptr()) == 0, lib_err()
        assert np.array_equal(c.read(), search_oracle(s, s[:n], "f32"))
    finally:
        c.release()
        c8.release()
    assert dev.getParam("debug.idle_dirty") == 0


def test_the_knobs_report_and_refuse(dev, C):
    from oclradixsort_amd import AdlHipError
    try:
        for v in (2, 16, C):
            dev.setParam("debug.search_lds_keys", v)
            assert dev.getParam("debug.search_lds_keys") == v
        dev.setParam("debug.search_lds_keys", 0)
        assert dev.getParam("debug.search_lds_keys") == C
        for v in (-1, 1, C + 1):
            with pytest.raises(AdlHipError, match="debug.search_lds_keys must be in"):
                dev.setParam("debug.search_lds_keys", v)
            assert dev.getParam("debug.search_lds_keys") == C
        dev.setParam("debug.search_grid", 7)
        assert dev.getParam("debug.search_grid") == 7
        with pytest.raises(AdlHipError, match="debug.search_grid must be >= 0"):
            dev.setParam("debug.search_grid", -1)
    finally:
        for k in KNOBS:
            dev.setParam(k, 0)


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


@pytest.mark.parametrize("right", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_searchsorted_and_bucketize_match_torch(sorter, dtype_name, right):
    dt = getattr(torch, dtype_name)
    for m, shape, span in ((3 * T + 7, (2 * T + 1,), 40), (5 * 4096 + 3, (3, 5, 7), 100000), (0, (4,), 3), (1, (1,), 1), (9, (0,), 3), (50, (2, 0, 3), 9)):
        n = int(np.prod(shape))
        seq = torch.sort(_torch_values(dt, m, 21 + m, span)).values
        vals = _torch_values(dt, n, 22 + n, span).reshape(shape)
        keep = seq.clone(), vals.clone()
        want = torch.searchsorted(seq, vals, right=right)
        got = sorter.searchsorted(seq, vals, right=right)
        assert got.dtype == torch.int64 and got.shape == vals.shape and torch.equal(got, want)
        got = sorter.searchsorted(seq, vals, side="right" if right else "left", out_int32=True)
        assert got.dtype == torch.int32 and torch.equal(got, torch.searchsorted(seq, vals, right=right, out_int32=True))
        got = sorter.bucketize(vals, seq, right=right)
        assert got.dtype == torch.int64 and torch.equal(got, torch.bucketize(vals, seq, right=right))
        got = sorter.bucketize(vals, seq, right=right, out_int32=True)
        assert got.dtype == torch.int32 and torch.equal(got, torch.bucketize(vals, seq, right=right, out_int32=True))
        assert torch.equal(seq, keep[0]) and torch.equal(vals, keep[1]), "an input was changed"
        if m:
            back = torch.flip(seq, (0,))                    # descending: what torch computes on the negated values
            got = sorter.searchsorted(back, vals, right=right, descending=True)
            assert torch.equal(got, torch.searchsorted(-back, -vals, right=right))


def test_torch_sorter_searchsorted_of_a_scalar_and_of_offset_views(sorter, monkeypatch):
    t = torch.sort(_torch_values(torch.float32, 3 * T + 2, 31)).values
    u = torch.sort(_torch_values(torch.int64, 2 * T + 4, 32)).values
    for seq, x in ((t, 1.25), (t, -100.0), (u, 3), (u, 1 << 40)):
        for right in (False, True):
            got = sorter.searchsorted(seq, x, right=right)
            want = torch.searchsorted(seq, torch.tensor(x, dtype=seq.dtype, device="cuda"), right=right)
            assert got.shape == () and got.dtype == torch.int64 and torch.equal(got, want)
            assert torch.equal(sorter.bucketize(x, seq, right=right), want)
    seen = []
    real = sorter.pprims.searchSorted
    monkeypatch.setattr(sorter.pprims, "searchSorted", lambda dev, s, *r, **k: (seen.append(s.m_ptr), real(dev, s, *r, **k))[1])
    for seq in (t[1:], t[3:T], u[1:]):
        assert seq.data_ptr() % 16
        vals = seq[5:T // 2]                                 # values at an odd offset too: they are copied, the sequence is not
        assert torch.equal(sorter.searchsorted(seq, vals), torch.searchsorted(seq, vals))
        assert seen[-1] == seq.data_ptr(), "the view was copied"
    assert torch.equal(sorter.searchsorted(t[::2], t[:100]), torch.searchsorted(t[::2].contiguous(), t[:100]))   # strided: copied


def test_torch_sorter_searchsorted_in_total_order(sorter):
    """NaN and -0: where it differs from torch, against the oracle"""
    bits = np.concatenate([SPECIALS[4], np.random.default_rng(4).integers(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32)])
    for order in ORDERS:
        seq = sort_bits(bits, "f32", order)
        needles = np.concatenate([SPECIALS[4], bits[::7]])
        ts = torch.from_numpy(seq.view(np.float32)).cuda()
        tx = torch.from_numpy(needles.view(np.float32)).cuda()
        for side in SIDES:
            got = sorter.searchsorted(ts, tx, right=side == RIGHT, descending=order == DESC)
            assert np.array_equal(got.cpu().numpy(), search_oracle(seq, needles, "f32", order, side).astype(np.int64))
    z = torch.tensor([-0.0, 0.0], device="cuda")
    assert sorter.searchsorted(z, z).tolist() == [0, 1] and sorter.searchsorted(z, z, right=True).tolist() == [1, 2]
    assert torch.searchsorted(z, z).tolist() == [0, 0]       # torch: equal


def test_torch_sorter_searchsorted_refuses_what_it_cannot_search(sorter):
    a = torch.arange(6, dtype=torch.int32, device="cuda")
    with pytest.raises(TypeError):
        sorter.searchsorted(a, a.to(torch.int64))
    with pytest.raises(TypeError):
        sorter.searchsorted(a.to(torch.float16), a.to(torch.float16))
    with pytest.raises(TypeError):
        sorter.searchsorted(a, [1, 2])
    with pytest.raises(TypeError):
        sorter.searchsorted(a, "3")
    with pytest.raises(ValueError):
        sorter.searchsorted(a.reshape(2, 3), a)
    with pytest.raises(ValueError):
        sorter.searchsorted(a, a, side="middle")
    with pytest.raises(ValueError):
        sorter.searchsorted(a, a, right=True, side="left")
    with pytest.raises(ValueError):
        sorter.searchsorted(a, a.cpu())
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        with pytest.raises(RuntimeError):
            sorter.searchsorted(a, a)
    assert sorter.searchsorted(a, a, right=True).tolist() == [1, 2, 3, 4, 5, 6]


def test_search_demo_device_path_matches_its_host_path():
    demo = os.path.join(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), "tests", "demo", "search_demo")

    def lines(args):
        r = subprocess.run([demo] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.strip()]

    device, host = lines(["--dump"]), lines(["--host", "--dump"])
    assert len(device) == len(host) and len([ln for ln in device if ln.startswith("DUMP ")]) == 4 * 2 * 2 * 3 * 6
    assert all(ln.startswith("[ OK ] Search.") for ln in device if ln.startswith("["))
    assert device == host
