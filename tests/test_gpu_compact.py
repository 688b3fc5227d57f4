"""Stream compaction on the GPU (include/adlhip.h "stream compaction"; oclradixsort_amd/csrc/compact_kernels.hpp;
Pprims.compactFlagged / compactIf; TorchSorter.masked_select / nonzero / select_if / partition).

The oracle is tests/compact_oracle.py (numpy; tests/test_compact_api.py checks it against a plain loop on the CPU).  Every case is
compared bit for bit.

Every output is sized exactly n, prefilled with sentinels and read back whole: the first S elements (all n of a partition) must be the
expected ones, everything behind them the sentinels.  Every device buffer carries guard bytes behind its payload -- flags, items, keys,
values, every output, the count word and the work buffer (sized exactly the reported bytes) -- and the inputs are compared with their
originals afterwards.  The handle's device state is idle after each case.

T2 / T4 below are the two tile sizes a width combination could use (2048 and 4096 elements; compact_kernels.hpp uses 2048 for all).
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from compact_oracle import BY_NAME, CMP_NAMES, CMPS, EQ, GE, GT, LE, LT, NE, SPECIALS, TYPE_IDS, compact_oracle, mask_from_cmp, mask_from_flags
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from test_gpu_reduce import Guarded, lib_err, sentinels

pytestmark = pytest.mark.gpu

T2, T4 = 2048, 4096
N40 = 40 * T4 + 3
SIZES = [1, 3, 4, 5, T2 - 1, T2, T2 + 1, T4 - 1, T4, T4 + 1, 2 * T4 + 3, N40]
GRIDS = [0, 1, 3, 7]
SENTINELS = 64
UDT = {0: None, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.compact_grid", 0)
    DeviceUtils.deallocate(d)


def scratch_bytes(dev, n):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_compact_scratch_bytes(dev._h, n, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def random_bits(udt, n, rng, specials=True):
    w = np.dtype(udt).itemsize
    v = np.frombuffer(rng.bytes(w * max(n, 1)), dtype=udt)[:n].copy()
    if specials and n >= 64:
        where = rng.integers(0, n, size=SPECIALS[w].size * 3)
        v[where] = np.tile(SPECIALS[w], 3)
    return v


class Case:
    """the device side of a series of calls on the same inputs: guarded inputs, sentinel-filled outputs sized exactly n, the count
    word, a work buffer of exactly the reported bytes.  ins / outs: {name: array} / {name: dtype}"""

    def __init__(self, dev, n, ins, outs, fill=None):
        self.dev, self.n, self.ins = dev, n, ins
        self.din = {k: Guarded(dev, v, guard_bytes=SENTINELS * v.dtype.itemsize, seed=5 + i) for i, (k, v) in enumerate(ins.items())}
        self.sent = {k: sentinels(dt, n, 0xa5a5a5a5a5a5a5a5 + 77 * i) for i, (k, dt) in enumerate(outs.items())}
        self.sent["count"] = np.array([0xdeadbeef], np.uint32)
        self.dout = {k: Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=20 + i) for i, (k, s) in enumerate(self.sent.items())}
        self.work = Guarded(dev, nbytes=scratch_bytes(dev, n), seed=8, fill=fill)

    def reset(self):
        for k, s in self.sent.items():
            self.dout[k].buf.write(s.view(np.uint8))

    def inp(self, name):
        return self.din[name].ptr() if name in self.din else None

    def out(self, name):
        return self.dout[name].ptr() if name in self.dout else None

    def check(self, s, exp, partition, what):
        """exp: {output name: the expected first S (partition: n) elements}"""
        got = {k: b.read(self.sent[k].dtype) for k, b in self.dout.items()}
        assert int(got["count"][0]) == s, "%s: %d selected, expected %d" % (what, int(got["count"][0]), s)
        m = self.n if partition else s
        for k, e in exp.items():
            g = got[k]
            assert e.size == m
            if not np.array_equal(g[:m], e):
                bad = np.flatnonzero(g[:m] != e)
                raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                    what, k, bad.size, m, bad[0], int(g[bad[0]]), int(e[bad[0]])))
            assert np.array_equal(g[m:], self.sent[k][m:]), "%s: %s was written at index %d or beyond" % (what, k, m)
        self.work.check_guard()
        for k, v in self.ins.items():
            assert np.array_equal(self.din[k].read(v.dtype), v), "%s: input %s was changed" % (what, k)
        assert self.dev.getParam("debug.idle_dirty") == 0
        return got

    def untouched(self):
        for k, b in self.dout.items():
            assert np.array_equal(b.read(self.sent[k].dtype), self.sent[k]), "%s was written" % k
        for k, v in self.ins.items():
            assert np.array_equal(self.din[k].read(v.dtype), v), "input %s was changed" % k
        self.work.check_guard()

    def release(self):
        for b in list(self.din.values()) + list(self.dout.values()) + [self.work]:
            b.release()


def call_flagged(dev, c, item_bytes, partition, n=None, work_bytes=None):
    return _lib.load().adlhip_compact_flagged(dev._h, item_bytes, c.inp("items"), c.inp("flags"), c.n if n is None else n, partition, c.out("items"),
                                              c.out("index"), c.out("count"), c.work.ptr(), c.work.nbytes if work_bytes is None else work_bytes)


def call_if(dev, c, kname, cmp, tbits, value_bytes, partition):
    t = np.array([tbits], dtype=BY_NAME[kname][3])
    return _lib.load().adlhip_compact_if_typed(dev._h, BY_NAME[kname][1], cmp, t.ctypes.data_as(ctypes.c_void_p), c.inp("keys"), value_bytes,
                                               c.inp("vals"), c.n, partition, c.out("keys"), c.out("vals"), c.out("index"), c.out("count"),
                                               c.work.ptr(), c.work.nbytes)


def run_flagged(dev, flags, items, outs=("items", "index"), partitions=(0, 1), grid=0, fill=None):
    """adlhip_compact_flagged on (flags, items or None) with every check of the memory contract, for each partition mode"""
    n = flags.size
    ins = {"flags": flags.view(np.uint8)}
    ib = 0
    if items is not None:
        ins["items"] = items
        ib = items.dtype.itemsize
    odt = {k: (items.dtype if k == "items" else np.uint32) for k in outs}
    c = Case(dev, n, ins, odt, fill=fill)
    dev.setParam("debug.compact_grid", grid)
    res = None
    try:
        for partition in partitions:
            c.reset()
            what = "flagged item_bytes %d outs %s n %d grid %d partition %d" % (ib, "+".join(outs), n, grid, partition)
            rc = call_flagged(dev, c, ib, partition)
            assert rc == 0, what + ": " + lib_err()
            s, index, arrays = compact_oracle(mask_from_flags(flags), partition, [items] if items is not None else [])
            exp = {"index": index}
            if items is not None:
                exp["items"] = arrays[0]
            res = c.check(s, {k: exp[k] for k in outs}, partition, what)
    finally:
        dev.setParam("debug.compact_grid", 0)
        c.release()
    return res


def run_if(dev, kname, kbits, cmps, thresholds, vals=None, outs=("keys", "vals", "index"), partitions=(0, 1), grid=0, fill=None):
    """adlhip_compact_if_typed for every (cmp, threshold, partition mode) on one set of device buffers; returns {(cmp, threshold,
    partition): the index output}"""
    n = kbits.size
    ins = {"keys": kbits}
    vb = 0
    if vals is not None:
        ins["vals"] = vals
        vb = vals.dtype.itemsize
    outs = tuple(k for k in outs if k != "vals" or vals is not None)
    odt = {k: {"keys": kbits.dtype, "vals": vals.dtype if vals is not None else None, "index": np.uint32}[k] for k in outs}
    c = Case(dev, n, ins, odt, fill=fill)
    dev.setParam("debug.compact_grid", grid)
    res = {}
    try:
        for cmp in cmps:
            for t in thresholds:
                for partition in partitions:
                    c.reset()
                    what = "if %s %s %#x value_bytes %d n %d grid %d partition %d" % (kname, CMP_NAMES[cmp], int(t), vb, n, grid, partition)
                    rc = call_if(dev, c, kname, cmp, t, vb, partition)
                    assert rc == 0, what + ": " + lib_err()
                    s, index, arrays = compact_oracle(mask_from_cmp(kbits, kname, cmp, t), partition, [kbits] + ([vals] if vals is not None else []))
                    exp = {"index": index, "keys": arrays[0]}
                    if vals is not None:
                        exp["vals"] = arrays[1]
                    got = c.check(s, {k: exp[k] for k in outs}, partition, what)
                    if "index" in got:
                        res[(cmp, int(t), partition)] = got["index"][:n if partition else s].copy()
    finally:
        dev.setParam("debug.compact_grid", 0)
        c.release()
    return res


# ---------------------------------------------------------------------------------------------
# sizes x grids
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_grids(dev, n, grid):
    rng = np.random.default_rng(1000 + n + grid)
    flags = (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    run_flagged(dev, flags, random_bits(np.uint32, n, rng), grid=grid)
    run_flagged(dev, flags, random_bits(np.uint64, n, rng), grid=grid)
    kbits = random_bits(np.uint32, n, rng)
    run_if(dev, "f32", kbits, [LT], [kbits[n // 2]], vals=random_bits(np.uint64, n, rng), grid=grid)
    k64 = random_bits(np.uint64, n, rng)
    run_if(dev, "i64", k64, [GE], [k64[n // 2]], vals=random_bits(np.uint32, n, rng), grid=grid)


def test_a_chunk_of_more_than_one_tile_on_the_default_grid(dev):
    n = (1 << 23) + 5
    rng = np.random.default_rng(23)
    assert n // T4 > 4 * int(dev.info.compute_units)      # more tiles, of either size, than workgroups
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    run_flagged(dev, flags, np.arange(n, dtype=np.uint32) * np.uint32(2654435761), partitions=(0,))
    kbits = random_bits(np.uint32, n, rng)
    run_if(dev, "i32", kbits, [LT], [np.uint32(12345)], vals=None, partitions=(1,))


# ---------------------------------------------------------------------------------------------
# flag patterns
# ---------------------------------------------------------------------------------------------
def _pattern(name, n, rng):
    f = np.zeros(n, np.uint8)
    i = np.arange(n)
    if name == "none":
        pass
    elif name == "all":
        f[:] = 1
    elif name == "first":
        f[0] = 1
    elif name == "last":
        f[-1] = 1
    elif name == "alternating":
        f[::2] = 1
    elif name == "tile_edges":                      # the first and the last element of every tile, both tile sizes
        f[(i % T2 == 0) | (i % T2 == T2 - 1)] = 1
    elif name == "tiles_2048":                      # whole tiles empty beside whole tiles full
        f[(i // T2) % 2 == 1] = 1
    elif name == "tiles_4096":
        f[(i // T4) % 2 == 0] = 1
    elif name == "chunk_empty":                     # grid 7: 81 tiles of 2048 (41 of 4096) in chunks of 12 (6); the third chunk is empty
        f[:] = rng.random(n) < 0.5
        f[2 * 12 * T2:3 * 12 * T2] = 0
    elif name.startswith("p"):
        f[:] = rng.random(n) < float(name[1:])
    elif name.startswith("byte"):
        f[rng.random(n) < 0.5] = int(name[4:], 16)
    else:
        raise KeyError(name)
    return f


PATTERNS = ["none", "all", "first", "last", "alternating", "tile_edges", "tiles_2048", "tiles_4096", "chunk_empty", "p0.01", "p0.5", "p0.99",
            "byte02", "byte80", "byteff"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_flag_patterns(dev, pattern):
    rng = np.random.default_rng(PATTERNS.index(pattern))
    flags = _pattern(pattern, N40, rng)
    items = random_bits(np.uint64, N40, rng)
    for grid in (0, 7):
        run_flagged(dev, flags, items, grid=grid)
    small = _pattern(pattern, 5, rng) if pattern not in ("chunk_empty",) else None
    if small is not None:
        run_flagged(dev, small, random_bits(np.uint32, 5, rng))


# (item_bytes 0 has no items to write: test_refusals_enqueue_nothing covers the other two combinations)
@pytest.mark.parametrize("item_bytes,outs", [(0, ("index",))] + [(b, o) for b in (4, 8) for o in (("items",), ("index",), ("items", "index"))],
                         ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_flagged_outputs(dev, item_bytes, outs):
    n = 3 * T4 + 5
    rng = np.random.default_rng(300 + item_bytes)
    flags = (rng.random(n) < 0.3).astype(np.uint8)
    items = random_bits(UDT[item_bytes], n, rng) if item_bytes else None
    for grid in (0, 3):
        run_flagged(dev, flags, items, outs=outs, grid=grid)   # partition 0 and 1


# ---------------------------------------------------------------------------------------------
# the if form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmp", CMPS, ids=[CMP_NAMES[c] for c in CMPS])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_if_every_key_type_and_cmp_with_special_patterns(dev, kname, cmp):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    n = 2 * T4 + 3
    rng = np.random.default_rng(400 + BY_NAME[kname][1])
    kbits = random_bits(udt, n, rng)
    kbits[rng.integers(0, n, size=n // 3)] = SPECIALS[w][rng.integers(0, SPECIALS[w].size, size=n // 3)]   # specials that repeat
    thresholds = np.concatenate([SPECIALS[w], kbits[100:102]])
    run_if(dev, kname, kbits, [cmp], thresholds, outs=("keys", "index"), partitions=(0,), grid=3)
    run_if(dev, kname, kbits, [cmp], thresholds[::5], outs=("keys",), partitions=(1,))


@pytest.mark.parametrize("vb", [0, 4, 8])
@pytest.mark.parametrize("kname", ["f32", "i64"])
def test_if_value_widths_with_each_key_width(dev, kname, vb):
    udt = BY_NAME[kname][3]
    n = 3 * T4 + 5
    rng = np.random.default_rng(500 + vb)
    kbits = random_bits(udt, n, rng)
    vals = random_bits(UDT[vb], n, rng) if vb else None
    for outs in (("keys", "vals", "index"), ("vals",), ("index",), ("keys",)):
        if outs == ("vals",) and not vb:
            continue
        for grid in (0, 7):
            run_if(dev, kname, kbits, [LE, NE], [kbits[7]], vals=vals, outs=outs, grid=grid)


@pytest.mark.parametrize("kname", TYPE_IDS)
def test_complementary_comparisons_partition_the_input(dev, kname):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    n = T4 + T2 + 7
    rng = np.random.default_rng(600 + BY_NAME[kname][1])
    kbits = random_bits(udt, n, rng)
    kbits[::5] = SPECIALS[w][3]
    thresholds = [SPECIALS[w][3], SPECIALS[w][0], SPECIALS[w][10], kbits[1]]
    res = run_if(dev, kname, kbits, CMPS, thresholds, outs=("index",), partitions=(0,), grid=3)
    for t in thresholds:
        for a, b in ((LT, GE), (EQ, NE), (LE, GT)):
            x, y = res[(a, int(t), 0)], res[(b, int(t), 0)]
            assert np.array_equal(np.sort(np.concatenate([x, y])), np.arange(n, dtype=np.uint32)), (kname, a, b, hex(int(t)))
            assert (np.diff(x.astype(np.int64)) > 0).all() and (np.diff(y.astype(np.int64)) > 0).all()
    assert res[(EQ, int(SPECIALS[w][3]), 0)].size >= n // 5


def test_partition_is_a_permutation_in_two_ordered_halves(dev):
    n = N40
    rng = np.random.default_rng(77)
    flags = (rng.random(n) < 0.37).astype(np.uint8)
    got = run_flagged(dev, flags, None, outs=("index",), partitions=(1,), grid=7)
    index, s = got["index"], int(got["count"][0])
    assert s == int(flags.sum()) and np.array_equal(np.sort(index), np.arange(n, dtype=np.uint32))
    assert (np.diff(index[:s].astype(np.int64)) > 0).all() and (np.diff(index[s:].astype(np.int64)) > 0).all()
    assert flags[index[:s]].all() and not flags[index[s:]].any()


# ---------------------------------------------------------------------------------------------
# the work buffer
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    n = 5 * T4 + 9
    rng = np.random.default_rng(81)
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    items = random_bits(np.uint32, n, rng)
    kbits = random_bits(np.uint64, n, rng)
    for fill in (0x00, 0xff):
        for grid in (0, 3):
            run_flagged(dev, flags, items, grid=grid, fill=fill)
            run_if(dev, "f64", kbits, [GT], [kbits[3]], vals=items, grid=grid, fill=fill)


def test_scratch_bytes_follow_the_formula_and_one_byte_short_is_refused(dev):
    cus = int(dev.info.compute_units)
    want = (16 * cus + 255) // 256 * 256
    for n in (0, 1, 2049, N40, 1 << 30, 0xFFF00000):
        assert scratch_bytes(dev, n) == want
    sz = ctypes.c_size_t()
    assert _lib.load().adlhip_compact_scratch_bytes(dev._h, 1 << 32, ctypes.byref(sz)) == 1
    n = 5000
    rng = np.random.default_rng(82)
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    c = Case(dev, n, {"flags": flags, "items": random_bits(np.uint32, n, rng)}, {"items": np.uint32, "index": np.uint32})
    k = Case(dev, n, {"keys": random_bits(np.uint32, n, rng)}, {"keys": np.uint32})
    try:
        assert call_flagged(dev, c, 4, 0, work_bytes=want - 1) == 1
        assert str(want) in lib_err(), lib_err()
        t = np.array([5], np.uint32)
        rc = _lib.load().adlhip_compact_if_typed(dev._h, 0, LT, t.ctypes.data_as(ctypes.c_void_p), k.inp("keys"), 0, None, n, 0, k.out("keys"), None,
                                                 None, k.out("count"), k.work.ptr(), want - 1)
        assert rc == 1 and str(want) in lib_err(), lib_err()
        c.untouched()
        k.untouched()
    finally:
        c.release()
        k.release()


# ---------------------------------------------------------------------------------------------
# refusals, n == 0
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    n = 5000
    rng = np.random.default_rng(91)
    flags = (rng.random(n) < 0.5).astype(np.uint8)
    items = random_bits(np.uint32, n, rng)
    vals = random_bits(np.uint64, n, rng)
    c = Case(dev, n, {"flags": flags, "items": items, "vals": vals}, {"items": np.uint32, "vals": np.uint64, "index": np.uint32})
    wb = c.work.nbytes
    null = ctypes.c_void_p(0)
    t = np.array([5], np.uint32)
    tp = t.ctypes.data_as(ctypes.c_void_p)
    count = c.out("count")

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    def flagged(item_bytes=4, i=0, f=0, m=n, partition=0, o=0, x=0, cnt=0, work=0, work_bytes=wb):
        """0 = the proper buffer; anything else replaces it"""
        return lib.adlhip_compact_flagged(dev._h, item_bytes, c.inp("items") if i == 0 else i, c.inp("flags") if f == 0 else f, m, partition,
                                          c.out("items") if o == 0 else o, c.out("index") if x == 0 else x, count if cnt == 0 else cnt,
                                          c.work.ptr() if work == 0 else work, work_bytes)

    def cif(key_type=0, cmp=LT, th=0, k=0, value_bytes=8, v=0, m=n, partition=0, ko=0, vo=0, x=0, cnt=0, work=0, work_bytes=wb):
        return lib.adlhip_compact_if_typed(dev._h, key_type, cmp, tp if th == 0 else th, c.inp("items") if k == 0 else k, value_bytes,
                                           c.inp("vals") if v == 0 else v, m, partition, c.out("items") if ko == 0 else ko,
                                           c.out("vals") if vo == 0 else vo, c.out("index") if x == 0 else x, count if cnt == 0 else cnt,
                                           c.work.ptr() if work == 0 else work, work_bytes)

    try:
        refused(flagged(f=null), "NULL flags")
        refused(flagged(i=null), "NULL items with item_bytes 4")
        refused(flagged(cnt=null), "NULL count word")
        refused(flagged(work=null), "NULL work")
        refused(flagged(o=null, x=null), "no output at all")
        refused(flagged(item_bytes=0, i=null, o=null, x=null), "no output at all, positions only")
        refused(flagged(item_bytes=0), "item_bytes 0 with item arrays")
        for bad in (-1, 1, 2, 16):
            refused(flagged(item_bytes=bad), "item_bytes %d" % bad)
        for bad in (-1, 2):
            refused(flagged(partition=bad), "partition %d" % bad)
            refused(cif(partition=bad), "partition %d" % bad)
        refused(flagged(f=c.din["flags"].ptr(8), m=n - 8), "misaligned flags")
        refused(flagged(i=c.din["items"].ptr(4), m=n - 1), "misaligned items")
        refused(flagged(o=c.dout["items"].ptr(8), m=n - 2), "misaligned items out")
        refused(flagged(x=c.dout["index"].ptr(4), m=n - 1), "misaligned index out")
        refused(flagged(cnt=ctypes.c_void_p(count.value + 2)), "misaligned count word")
        refused(flagged(work=c.work.ptr(4), work_bytes=wb - 4), "misaligned work")
        refused(flagged(o=c.din["items"].ptr(0)), "items out is items in")
        refused(flagged(o=c.din["items"].ptr(16), m=n - 4), "items out overlaps items in")
        refused(flagged(x=c.din["flags"].ptr(16), m=n // 4 - 4), "index out overlaps the flags")
        refused(flagged(cnt=c.din["items"].ptr(64)), "the count word lies in the items")
        refused(flagged(cnt=c.din["flags"].ptr(64)), "the count word lies in the flags")
        refused(flagged(m=1 << 32), "n = 2^32")
        assert str(wb) in refused(flagged(work_bytes=wb - 1), "work one byte short")

        refused(cif(k=null), "NULL keys")
        refused(cif(v=null), "NULL values with value_bytes 8")
        refused(cif(th=null), "NULL threshold")
        refused(cif(cnt=null), "NULL count word")
        refused(cif(work=null), "NULL work")
        refused(cif(ko=null, vo=null, x=null), "no output at all")
        refused(cif(value_bytes=0), "value_bytes 0 with value arrays")
        for bad in (-1, 6, 99):
            refused(cif(key_type=bad), "key_type %d" % bad)
            refused(cif(cmp=bad), "cmp %d" % bad)
        for bad in (-1, 2, 16):
            refused(cif(value_bytes=bad), "value_bytes %d" % bad)
        refused(cif(k=c.din["items"].ptr(4), m=n - 1), "misaligned keys")
        refused(cif(v=c.din["vals"].ptr(8), m=n - 1), "misaligned values")
        refused(cif(ko=c.dout["items"].ptr(4), m=n - 1), "misaligned keys out")
        refused(cif(vo=c.dout["vals"].ptr(8), m=n - 1), "misaligned values out")
        refused(cif(ko=c.din["items"].ptr(0)), "keys out is keys in")
        refused(cif(vo=c.din["vals"].ptr(16), m=n - 2), "values out overlaps values in")
        refused(cif(ko=c.din["vals"].ptr(16), m=n - 2), "keys out overlaps values in")
        refused(cif(x=c.din["items"].ptr(16), m=n - 4), "index out overlaps keys in")
        refused(cif(cnt=c.din["vals"].ptr(64)), "the count word lies in the values")
        refused(cif(m=1 << 32), "n = 2^32")
        assert str(wb) in refused(cif(work_bytes=wb - 1), "work one byte short")
        c.untouched()
        assert dev.getParam("debug.idle_dirty") == 0
        # the proper calls go through
        assert flagged(partition=1) == 0, lib_err()
        s, index, (eitems,) = compact_oracle(mask_from_flags(flags), True, [items])
        assert int(c.dout["count"].read(np.uint32)[0]) == s
        assert np.array_equal(c.dout["items"].read(np.uint32), eitems) and np.array_equal(c.dout["index"].read(np.uint32), index)
        assert cif() == 0, lib_err()
        s, index, (ekeys, evals) = compact_oracle(mask_from_cmp(items, "u32", LT, 5), False, [items, vals])
        assert int(c.dout["count"].read(np.uint32)[0]) == s and np.array_equal(c.dout["vals"].read(np.uint64)[:s], evals)
    finally:
        c.release()


def test_empty_input_clears_only_the_count_word(dev):
    lib = _lib.load()
    n = 100
    c = Case(dev, n, {"flags": np.ones(n, np.uint8), "items": np.arange(n, dtype=np.uint32)}, {"items": np.uint32, "index": np.uint32})
    t = np.array([5], np.uint64)
    try:
        for call in (lambda: call_flagged(dev, c, 4, 0, n=0),
                     lambda: lib.adlhip_compact_flagged(dev._h, 0, None, None, 0, 1, None, c.out("index"), c.out("count"), None, 0),
                     lambda: lib.adlhip_compact_if_typed(dev._h, 0, LT, t.ctypes.data_as(ctypes.c_void_p), c.inp("items"), 0, None, 0, 0,
                                                         c.out("items"), None, None, c.out("count"), c.work.ptr(), c.work.nbytes),
                     lambda: lib.adlhip_compact_if_typed(dev._h, 5, NE, t.ctypes.data_as(ctypes.c_void_p), None, 0, None, 0, 1, None, None,
                                                         c.out("index"), c.out("count"), None, 0)):
            c.reset()
            assert call() == 0, lib_err()
            assert c.dout["count"].read(np.uint32)[0] == 0
            assert np.array_equal(c.dout["items"].read(np.uint32), c.sent["items"]) and np.array_equal(c.dout["index"].read(np.uint32), c.sent["index"])
            c.work.check_guard()
        # refusals come first even then
        c.reset()
        assert lib.adlhip_compact_flagged(dev._h, 4, c.inp("items"), c.inp("flags"), 0, 0, None, None, c.out("count"), c.work.ptr(), c.work.nbytes) == 1
        assert lib.adlhip_compact_flagged(dev._h, 4, c.inp("items"), c.inp("flags"), 0, 0, c.out("items"), None, None, c.work.ptr(), c.work.nbytes) == 1
        assert c.dout["count"].read(np.uint32)[0] == 0xdeadbeef
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        c.release()


# ---------------------------------------------------------------------------------------------
# call sequences, the Pprims mirror
# ---------------------------------------------------------------------------------------------
def test_two_different_calls_back_to_back_on_one_handle(dev):
    """nothing is remembered between calls: a flagged partition of n elements, then an if selection of other, fewer elements through the
    same work buffer, read back only after both were enqueued; then the other way round"""
    lib = _lib.load()
    rng = np.random.default_rng(55)
    n1, n2 = 6 * T4 + 1, T2 + 9
    flags = (rng.random(n1) < 0.6).astype(np.uint8)
    items = random_bits(np.uint64, n1, rng)
    kbits = random_bits(np.uint32, n2, rng)
    a = Case(dev, n1, {"flags": flags, "items": items}, {"items": np.uint64, "index": np.uint32})
    b = Case(dev, n2, {"keys": kbits}, {"keys": np.uint32, "index": np.uint32})
    t = np.array([kbits[5]], np.uint32)
    try:
        for order in ((0, 1), (1, 0)):
            a.reset()
            b.reset()
            for which in order:
                if which == 0:
                    rc = lib.adlhip_compact_flagged(dev._h, 8, a.inp("items"), a.inp("flags"), n1, 1, a.out("items"), a.out("index"), a.out("count"),
                                                    a.work.ptr(), a.work.nbytes)
                else:
                    rc = lib.adlhip_compact_if_typed(dev._h, 2, GT, t.ctypes.data_as(ctypes.c_void_p), b.inp("keys"), 0, None, n2, 0, b.out("keys"),
                                                     None, b.out("index"), b.out("count"), a.work.ptr(), a.work.nbytes)
                assert rc == 0, lib_err()
            s, index, (eitems,) = compact_oracle(mask_from_flags(flags), True, [items])
            a.check(s, {"items": eitems, "index": index}, True, "back to back: flagged")
            s, index, (ekeys,) = compact_oracle(mask_from_cmp(kbits, "f32", GT, kbits[5]), False, [kbits])
            b.check(s, {"keys": ekeys, "index": index}, False, "back to back: if")
    finally:
        a.release()
        b.release()


def test_pprims_mirror(dev):
    p = Pprims()
    n = 3 * T4 + 11
    rng = np.random.default_rng(66)
    flags = (rng.random(n) < 0.4).astype(np.uint8)
    fitems = random_bits(np.uint32, n, rng).view(np.float32)
    keys = random_bits(np.uint64, n, rng).view(np.int64)
    vals = random_bits(np.uint32, n, rng).view(np.int32)
    bufs = []

    def dbuf(a):
        b = Buffer(dev, a.size, a.dtype)
        b.write(a)
        bufs.append(b)
        return b

    try:
        bf, bi, bk, bv = dbuf(flags), dbuf(fitems), dbuf(keys), dbuf(vals)
        for partition in (False, True):
            r = p.compactFlagged(dev, bf, n, items=bi, partition=partition, indexOut=True)
            bufs.extend([r.items, r.index, r.count])
            s, index, (eitems,) = compact_oracle(mask_from_flags(flags), partition, [fitems.view(np.uint32)])
            m = n if partition else s
            assert int(r.count.toHost()[0]) == s and r.values is None
            assert np.array_equal(r.items.toHost().view(np.uint32)[:m], eitems) and np.array_equal(r.index.toHost()[:m], index)
        r = p.compactFlagged(dev, bf, n, indexOut=True)                         # positions only
        bufs.extend([r.index, r.count])
        assert r.items is None and np.array_equal(r.index.toHost()[:int(r.count.toHost()[0])], np.flatnonzero(flags).astype(np.uint32))
        th = keys[17]
        for cmp in ("lt", "ge", "eq", "!="):
            mine = Buffer(dev, n, np.int64)
            bufs.append(mine)
            r = p.compactIf(dev, bk, n, cmp, th, values=bv, keysOut=mine, indexOut=True)
            bufs.extend([r.values, r.index, r.count])
            assert r.items is mine
            code = {"lt": LT, "ge": GE, "eq": EQ, "!=": NE}[cmp]
            s, index, (ekeys, evals) = compact_oracle(mask_from_cmp(keys.view(np.uint64), "i64", code, th.view(np.uint64)), False,
                                                      [keys.view(np.uint64), vals.view(np.uint32)])
            assert int(r.count.toHost()[0]) == s
            assert np.array_equal(r.items.toHost().view(np.uint64)[:s], ekeys) and np.array_equal(r.values.toHost().view(np.uint32)[:s], evals)
            assert np.array_equal(r.index.toHost()[:s], index)
        r = p.compactIf(dev, bi, n, "gt", np.float32(0.0), keysOut=False, indexOut=True, partition=True)   # -0 is not above +0, +NaN is
        bufs.extend([r.index, r.count])
        s, index, _ = compact_oracle(mask_from_cmp(fitems.view(np.uint32), "f32", GT, np.uint32(0)), True, [])
        assert r.items is None and int(r.count.toHost()[0]) == s and np.array_equal(r.index.toHost(), index)
        assert np.array_equal(bf.toHost(), flags) and np.array_equal(bk.toHost(), keys)
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for b in bufs:
            b.release()
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


_DTYPES = ["int32", "int64", "float32", "float64"]


def _torch_values(dtype, shape, seed):
    """no NaN, no -0 (no zero at all among the floats)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-40, 40, shape, dtype=torch.int64, device="cuda", generator=g)
    if dtype.is_floating_point:
        return torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25
    return t.to(dtype)


@pytest.mark.parametrize("dtype_name", _DTYPES)
def test_torch_sorter_masked_select_partition_and_select_if_match_torch(sorter, dtype_name):
    dt = getattr(torch, dtype_name)
    t = _torch_values(dt, (7, 33, 41), 21)
    g = torch.Generator(device="cuda").manual_seed(22)
    mask = torch.rand(t.shape, device="cuda", generator=g) < 0.3
    keep_t, keep_m = t.clone(), mask.clone()
    for x, m in ((t, mask), (t[::2], mask[::2]), (t[:, 1:, :], mask[:, 1:, :]), (t.reshape(-1)[1:], mask.reshape(-1)[1:]), (t[:0], mask[:0])):
        got = sorter.masked_select(x, m)
        assert got.dtype == dt and torch.equal(got, torch.masked_select(x, m))
        assert torch.equal(sorter.masked_select(x, m.to(torch.uint8) * 7), torch.masked_select(x, m))
        out, s = sorter.partition(x, m)
        assert s == int(m.sum()) and torch.equal(out, torch.cat([x[m], x[~m]]))
    flat = t.reshape(-1)
    vals = _torch_values(torch.int64 if dt != torch.int64 else torch.float32, (flat.numel(),), 23)
    ops = {"lt": torch.lt, "le": torch.le, "gt": torch.gt, "ge": torch.ge, "eq": torch.eq, "ne": torch.ne}
    for th in (3, -5, 100, -100):
        thv = th * 0.25 if dt.is_floating_point else th
        for cmp, fn in ops.items():
            want = fn(flat, thv)
            got = sorter.select_if(flat, cmp, thv)
            assert got.dtype == dt and torch.equal(got, flat[want]), (cmp, thv)
        k, v, i = sorter.select_if(flat[1:], "<", thv, values=vals[1:], return_indices=True)
        want = flat[1:] < thv
        assert torch.equal(k, flat[1:][want]) and torch.equal(v, vals[1:][want]) and torch.equal(i, torch.nonzero(want).reshape(-1))
        assert i.dtype == torch.int64 and v.dtype == vals.dtype
    e = sorter.select_if(flat[:0], "lt", 1)
    assert e.numel() == 0 and e.dtype == dt
    assert torch.equal(t, keep_t) and torch.equal(mask, keep_m), "an input was changed"


def test_torch_sorter_nonzero_matches_torch(sorter):
    g = torch.Generator(device="cuda").manual_seed(31)
    for shape in ((50_003,), (7, 33, 41), (5, 0, 3), (0,)):
        mask = torch.rand(shape, device="cuda", generator=g) < 0.2
        for m in (mask, mask.to(torch.uint8) * 0x80):
            got = sorter.nonzero(m)
            assert got.dtype == torch.int64 and got.shape == torch.nonzero(mask).shape and torch.equal(got, torch.nonzero(mask))
    m3 = torch.rand((6, 10, 12), device="cuda", generator=g) < 0.5
    assert torch.equal(sorter.nonzero(m3[:, ::2, 1:]), torch.nonzero(m3[:, ::2, 1:]))
    assert torch.equal(sorter.nonzero(torch.zeros(9, dtype=torch.bool, device="cuda")), torch.zeros((0, 1), dtype=torch.int64, device="cuda"))
    assert sorter.nonzero(torch.ones(9, dtype=torch.bool, device="cuda")).reshape(-1).tolist() == list(range(9))


def test_torch_sorter_select_if_orders_nan_and_negative_zero_by_total_order(sorter):
    nan = float("nan")
    t = torch.tensor([1.0, -0.0, 0.0, nan, -nan, -1.0, float("inf")], dtype=torch.float32, device="cuda")
    t[4] = -t[3]     # a NaN with the sign bit set
    bits = lambda x: x.view(torch.int32).tolist()
    assert bits(sorter.select_if(t, "lt", 0.0)) == bits(t[[1, 4, 5]])            # -0 and -NaN are below +0 (torch: only -1)
    assert bits(sorter.select_if(t, "gt", float("inf"))) == bits(t[[3]])          # +NaN is above +inf (torch: nothing)
    assert bits(sorter.select_if(t, "eq", 0.0)) == bits(t[[2]])                   # bits: -0 is not +0
    assert bits(sorter.select_if(t, "eq", nan)) == bits(t[[3]])                   # a NaN equals itself


def test_torch_sorter_compactions_are_bound_to_their_stream(sorter, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.tensor([3, 1, 4, 1, 5, 9], dtype=torch.int32, device="cuda")
    m = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.bool, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "compactFlagged", boom)
        monkeypatch.setattr(sorter.pprims, "compactIf", boom)
        for call in (lambda: sorter.masked_select(t, m), lambda: sorter.nonzero(m), lambda: sorter.partition(t, m),
                     lambda: sorter.select_if(t, "lt", 4)):
            with pytest.raises(RuntimeError):
                call()
        monkeypatch.undo()
    assert sorter.masked_select(t, m).tolist() == [3, 4, 1]
    assert sorter.nonzero(m).tolist() == [[0], [2], [3]]
    out, s = sorter.partition(t, m)
    assert out.tolist() == [3, 4, 1, 1, 5, 9] and s == 3
    assert sorter.select_if(t, "ge", 4).tolist() == [4, 5, 9]
    for bad in (torch.zeros(6, dtype=torch.float16, device="cuda"), torch.zeros(6, dtype=torch.int32), [3, 1]):
        for call in (lambda b: sorter.masked_select(b, m), lambda b: sorter.partition(b, m), lambda b: sorter.select_if(b, "lt", 1)):
            with pytest.raises((TypeError, ValueError)):
                call(bad)
    for bad in (torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.bool), [True]):
        for call in (lambda b: sorter.masked_select(t, b), lambda b: sorter.nonzero(b)):
            with pytest.raises((TypeError, ValueError)):
                call(bad)
    with pytest.raises(ValueError):
        sorter.masked_select(t, m[:5])                                  # no broadcasting
    with pytest.raises(ValueError):
        sorter.masked_select(t.reshape(2, 3), m)
    with pytest.raises(ValueError):
        sorter.select_if(t, "less", 4)
    with pytest.raises(ValueError):
        sorter.select_if(t.reshape(2, 3), "lt", 4)
    with pytest.raises(ValueError):
        sorter.select_if(t, "lt", 4, values=t[:5])


def test_compact_demo_device_path_matches_its_host_path():
    import os
    import subprocess
    demo = os.path.join(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), "tests", "demo", "compact_demo")

    def lines(args):
        r = subprocess.run([demo] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.strip()]

    device, host = lines(["--dump"]), lines(["--host", "--dump"])
    assert len(device) == len(host) and len([ln for ln in device if ln.startswith("DUMP ")]) == 3 * 2 * (2 * 5 + 8 * 6)
    assert all(ln.startswith("[ OK ] Compact.") for ln in device if ln.startswith("["))
    assert device == host
