"""Unique keys, run lengths and inverse indices on the GPU (include/adlhip.h "unique keys, run lengths, inverse indices";
oclradixsort_amd/csrc/unique_kernels.hpp; Pprims.unique / runLengthEncode; TorchSorter.unique / unique_consecutive).

The oracle is numpy on the encoded ordinal (the order-preserving code of include/adlhip.h "typed keys"; descending: its complement):
np.unique(code, return_index=True, return_inverse=True, return_counts=True), offsets = [0] + cumsum(counts), keys compared as bit
patterns.  tests/test_unique_api.py checks on the CPU that return_index is the stable argsort's run heads, NaNs of both signs and +-0
included.  Everything is compared bit for bit, nothing is excluded, there is no tolerance.

Every output is prefilled with a sentinel pattern and read back whole: the first R elements (offsets: R + 1) must be the expected ones,
everything behind them the sentinels.  Every device buffer carries guard bytes behind its payload -- the input, every output (sized
exactly n, offsets n + 1), the count word and the work buffer (sized exactly the reported bytes) -- and the input is compared with its
original afterwards.

T below is the tile of the run stage (the selection kernels' tile): 256 threads x 4 vectors of 16 bytes = 4096 4-byte keys / 2048
8-byte keys; PER = the keys of one 16-byte vector.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib

pytestmark = pytest.mark.gpu

ASC, DESC = 0, 1
TYPES = [("u32", 0, np.uint32, np.uint32), ("i32", 1, np.int32, np.uint32), ("f32", 2, np.float32, np.uint32),
         ("u64", 3, np.uint64, np.uint64), ("i64", 4, np.int64, np.uint64), ("f64", 5, np.float64, np.uint64)]
BY_NAME = {t[0]: t for t in TYPES}
TYPE_IDS = [t[0] for t in TYPES]
ORDER_IDS = ["asc", "desc"]
SENTINELS = 64
TILE = {4: 4096, 8: 2048}
PER = {4: 4, 8: 2}
ALL = ("counts", "offsets", "first", "inverse")

SPECIALS = {
    4: np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff, 0x7f800000,
                 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00123, 0xffc00123, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff,
                 0xfffffffe, 0x3f800000, 0xbf800000], dtype=np.uint32),
    8: np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x0010000000000000,
                 0x8010000000000000, 0x7fefffffffffffff, 0xffefffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                 0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123, 0xfff8000000000123, 0x7ff0000000000001,
                 0xfff0000000000001, 0x7fffffffffffffff, 0xffffffffffffffff, 0xfffffffffffffffe, 0x3ff0000000000000,
                 0xbff0000000000000, 0x00000000ffffffff, 0x0000000100000000, 0xffffffff00000000], dtype=np.uint64),
}


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def encode(bits, name, order):
    w = bits.dtype.itemsize
    udt = bits.dtype.type
    sign = udt(1 << (8 * w - 1))
    ones = udt((1 << (8 * w)) - 1)
    e = bits.copy()
    if name[0] == "i":
        e ^= sign
    if name[0] == "f":
        e ^= np.where(bits & sign != 0, ones, sign).astype(udt)
    return ~e if order == DESC else e


def unique_oracle(bits, name, order):
    _, first, inverse, counts = np.unique(encode(bits, name, order), return_index=True, return_inverse=True, return_counts=True)
    return {"unique": bits[first], "counts": counts.astype(np.uint32), "first": first.astype(np.uint32),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), "inverse": inverse.reshape(-1).astype(np.uint32)}


def rle_oracle(bits):
    heads = np.flatnonzero(np.concatenate([[True], bits[1:] != bits[:-1]]))
    offsets = np.concatenate([heads, [bits.size]]).astype(np.uint32)
    return {"unique": bits[heads], "offsets": offsets, "counts": np.diff(offsets).astype(np.uint32)}


def tied_bits(udt, n, seed, values=None, specials=True):
    """n keys drawn from `values` random bit patterns (default: about n / 3, so that runs of every short length occur) and, where there
    is room, the special patterns"""
    rng = np.random.default_rng(seed)
    w = np.dtype(udt).itemsize
    m = max(1, n // 3) if values is None else values
    pool = np.frombuffer(rng.bytes(w * m), dtype=udt)
    if specials and n >= 8:
        pool = np.concatenate([pool, SPECIALS[w]])
    return np.ascontiguousarray(pool[rng.integers(0, pool.size, size=n)], dtype=udt)


def sentinels(dtype, count, salt):
    return (np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ np.uint64(salt)).astype(dtype)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("unique.algo", -1)
    d.setParam("debug.unique_grid", 0)
    DeviceUtils.deallocate(d)


def lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


class Guarded:
    """`payload` (taken as bytes) -- or nbytes of scratch, contents arbitrary unless `fill` is given -- on the device, followed by a
    guard of known bytes."""

    def __init__(self, dev, payload=None, nbytes=None, guard_bytes=256, seed=1, fill=None):
        self.dev = dev
        self.guard = np.random.default_rng(seed).integers(0, 256, size=guard_bytes, dtype=np.uint8)
        if payload is not None:
            body = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
            self.nbytes = body.size
            self.buf = Buffer(dev, self.nbytes + guard_bytes, np.uint8)
            self.buf.write(np.concatenate([body, self.guard]))
        else:
            self.nbytes = int(nbytes)
            self.buf = Buffer(dev, self.nbytes + guard_bytes, np.uint8)
            if fill is not None and self.nbytes:
                rc = _lib.load().adlhip_memset(dev._h, self.buf.ptr(), int(fill), self.nbytes)
                assert rc == 0, lib_err()
            self.buf.write(self.guard, dstOffsetNElems=self.nbytes)

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.buf.m_ptr + offset)

    def check_guard(self):
        got = np.empty(self.guard.size, np.uint8)
        self.buf.read(got, srcOffsetNElems=self.nbytes)
        DeviceUtils.waitForCompletion(self.dev)
        assert np.array_equal(got, self.guard), "bytes behind the buffer were written"

    def read(self, dtype):
        raw = self.buf.toHost()
        assert np.array_equal(raw[self.nbytes:], self.guard), "bytes behind the buffer were written"
        return raw[:self.nbytes].view(dtype)

    def release(self):
        self.buf.release()


def unique_bytes(dev, kt, n, want_index):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_unique_scratch_bytes(dev._h, kt, n, want_index, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def rle_bytes(dev, key_bytes, n):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_run_length_encode_scratch_bytes(dev._h, key_bytes, n, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Outputs:
    """sentinel-filled outputs of one call: `unique` and the count word always, the others where named"""

    SIZES = {"counts": 0, "offsets": 1, "first": 0, "inverse": 0}   # elements beyond n

    def __init__(self, dev, udt, n, names):
        self.n, self.udt = n, udt
        self.sent = {"unique": sentinels(udt, n, 0xa5a5a5a5a5a5a5a5), "count": np.array([0xdeadbeef], np.uint32)}
        for i, name in enumerate(names):
            self.sent[name] = sentinels(np.uint32, n + self.SIZES[name], 0x5a5a5a5a + i)
        self.bufs = {}
        for i, (name, s) in enumerate(self.sent.items()):
            self.bufs[name] = Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=10 + i)

    def ptr(self, name):
        return self.bufs[name].ptr() if name in self.bufs else None

    def check(self, exp, what):
        """the first R elements (offsets: R + 1) are the expected ones, the rest the sentinels; inverse is written whole"""
        got = {name: b.read(self.sent[name].dtype) for name, b in self.bufs.items()}
        r = int(got["count"][0])
        assert r == exp["unique"].size, "%s: %d runs, expected %d" % (what, r, exp["unique"].size)
        for name, g in got.items():
            if name == "count":
                continue
            m = self.n if name == "inverse" else r + self.SIZES.get(name, 0)
            assert np.array_equal(g[:m], exp[name]), "%s: %s differs" % (what, name)
            assert np.array_equal(g[m:], self.sent[name][m:]), "%s: %s was written at index %d or beyond" % (what, name, m)

    def untouched(self):
        for name, b in self.bufs.items():
            assert np.array_equal(b.read(self.sent[name].dtype), self.sent[name]), "%s was written" % name

    def release(self):
        for b in self.bufs.values():
            b.release()


def check_unique(dev, name, bits, order, names=ALL, algo=-1, grid=0, exp=None, work=None, fill=None):
    kt, udt, n = BY_NAME[name][1], bits.dtype.type, bits.size
    exp = unique_oracle(bits, name, order) if exp is None else exp
    dev.setParam("unique.algo", algo)
    dev.setParam("debug.unique_grid", grid)
    index = algo == 1 or "first" in names or "inverse" in names
    wb = unique_bytes(dev, kt, n, 1 if index else 0)
    inp = Guarded(dev, bits, guard_bytes=SENTINELS * bits.dtype.itemsize, seed=5)
    out = Outputs(dev, udt, n, names)
    own = work is None
    w = Guarded(dev, nbytes=wb, seed=8, fill=fill) if own else work
    what = "%s order %d n %d algo %d grid %d" % (name, order, n, algo, grid)
    try:
        rc = _lib.load().adlhip_unique_typed(dev._h, kt, order, inp.ptr(), n, out.ptr("unique"), out.ptr("counts"), out.ptr("offsets"),
                                             out.ptr("first"), out.ptr("inverse"), out.ptr("count"), w.ptr(), w.nbytes)
        assert rc == 0, lib_err()
        out.check(exp, what)
        w.check_guard()
        assert np.array_equal(inp.read(bits.dtype), bits), what + ": d_keys_in was changed"
    finally:
        dev.setParam("unique.algo", -1)
        dev.setParam("debug.unique_grid", 0)
        inp.release()
        out.release()
        if own:
            w.release()
    return exp


def check_rle(dev, bits, names=("counts", "offsets"), grid=0, exp=None, fill=None):
    udt, n, kb = bits.dtype.type, bits.size, bits.dtype.itemsize
    exp = rle_oracle(bits) if exp is None else exp
    dev.setParam("debug.unique_grid", grid)
    wb = rle_bytes(dev, kb, n)
    inp = Guarded(dev, bits, guard_bytes=SENTINELS * kb, seed=5)
    out = Outputs(dev, udt, n, names)
    w = Guarded(dev, nbytes=wb, seed=8, fill=fill)
    what = "run-length encode, %d-byte keys, n %d grid %d" % (kb, n, grid)
    try:
        rc = _lib.load().adlhip_run_length_encode(dev._h, kb, inp.ptr(), n, out.ptr("unique"), out.ptr("counts"), out.ptr("offsets"),
                                                  out.ptr("count"), w.ptr(), w.nbytes)
        assert rc == 0, lib_err()
        out.check(exp, what)
        w.check_guard()
        assert np.array_equal(inp.read(bits.dtype), bits), what + ": d_keys_in was changed"
    finally:
        dev.setParam("debug.unique_grid", 0)
        for b in (inp, w):
            b.release()
        out.release()
    return exp


# ---------------------------------------------------------------------------------------------
# every type, both orders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_every_type_and_order_with_special_patterns(dev, name, kt, dt, udt, order):
    bits = tied_bits(udt, 30_011, seed=100 + kt, values=500)
    assert np.isin(SPECIALS[bits.dtype.itemsize], bits).all()
    exp = check_unique(dev, name, bits, order)                                      # the index path, every output
    check_unique(dev, name, bits, order, names=("counts", "offsets"), exp=exp)      # the keys path
    check_unique(dev, name, bits, order, names=(), exp=exp)                         # unique and the count alone
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# sizes: vector, tile and sort-path edges
# ---------------------------------------------------------------------------------------------
def _sizes(w):
    t, p = TILE[w], PER[w]
    return [1, 2, p - 1, p, p + 1, t - 1, t, t + 1, 2 * t + 3, 100_003, (2 << 20) + 5, (4 << 20) + 3]


_SIZE_CASES = sorted(set((name, n) for name, w in (("f32", 4), ("i64", 8)) for n in _sizes(w)))


@pytest.mark.parametrize("name,n", _SIZE_CASES, ids=["%s-%d" % c for c in _SIZE_CASES])
def test_sizes(dev, name, n):
    udt = BY_NAME[name][3]
    bits = tied_bits(udt, n, seed=7 * n + 1)
    big = n > (1 << 20)
    if big:   # (the large sizes: one order per path, to stay within a few seconds)
        check_unique(dev, name, bits, DESC)
        check_unique(dev, name, bits, ASC, names=("counts",))
    else:
        for order in (ASC, DESC):
            exp = check_unique(dev, name, bits, order)
            check_unique(dev, name, bits, order, names=("counts",), exp=exp)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# run shapes x grids
# ---------------------------------------------------------------------------------------------
def _run_shapes(w):
    """sorted keys (ascending, unsigned) with a chosen run structure, as run lengths"""
    t = TILE[w]
    rng = np.random.default_rng(21)
    return {
        "all-equal": [3 * t + 5],
        "all-distinct": [1] * (2 * t + 7),
        "one-tile-each": [t] * 5,                                   # heads sit on tile starts
        "straddling": [t - 1, 3, t + 2, 1, 1, 2 * t - 5, 7, t // 2, t, t - 3, 5],   # runs across tile and chunk boundaries
        "whole-tiles-without-heads": [1, 3 * t + t // 2, 2, 1, 5, t // 3],          # tiles 1 and 2 hold no head
        "random-lengths": rng.integers(1, t // 2, size=14).tolist(),
    }


_SHAPES = [(w, s) for w in (4, 8) for s in _run_shapes(4)]


@pytest.mark.parametrize("grid", [0, 1, 3], ids=["grid-default", "grid-1", "grid-3"])
@pytest.mark.parametrize("w,shape", _SHAPES, ids=["%d-byte-%s" % c for c in _SHAPES])
def test_run_shapes_and_grids(dev, w, shape, grid):
    udt = np.uint32 if w == 4 else np.uint64
    lengths = np.array(_run_shapes(w)[shape], dtype=np.int64)
    rng = np.random.default_rng(22)
    values = np.sort(np.frombuffer(rng.bytes(w * lengths.size * 2), dtype=udt))
    values = np.unique(values)[:lengths.size]
    assert values.size == lengths.size
    bits = np.repeat(values, lengths)
    exp = check_rle(dev, bits, grid=grid)
    assert np.array_equal(exp["counts"].astype(np.int64), lengths)
    check_rle(dev, bits, names=("counts",), grid=grid, exp=exp)        # the offsets live in the work buffer
    check_rle(dev, bits, names=(), grid=grid, exp=exp)
    name = "u32" if w == 4 else "u64"
    # the same keys shuffled, through both paths of unique
    shuffled = bits[rng.permutation(bits.size)]
    uexp = check_unique(dev, name, shuffled, ASC, grid=grid)
    assert np.array_equal(uexp["unique"], values) and np.array_equal(uexp["counts"].astype(np.int64), lengths)
    check_unique(dev, name, shuffled, ASC, names=("counts", "offsets"), grid=grid, exp=uexp)
    check_unique(dev, "i32" if w == 4 else "f64", shuffled, DESC, grid=grid)
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("grid", [0, 1, 3], ids=["grid-default", "grid-1", "grid-3"])
def test_few_workgroups_take_many_tiles(dev, grid):
    for name in ("f32", "f64"):
        bits = tied_bits(BY_NAME[name][3], 100_003, seed=33, values=3000)
        exp = check_unique(dev, name, bits, DESC, grid=grid)
        check_unique(dev, name, bits, DESC, names=("offsets",), grid=grid, exp=exp)
    dev.setParam("debug.unique_grid", 3)
    assert dev.getParam("debug.unique_grid") == 3
    dev.setParam("debug.unique_grid", 0)
    with pytest.raises(Exception):
        dev.setParam("debug.unique_grid", -1)


# ---------------------------------------------------------------------------------------------
# the two paths agree
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u32", "f32", "i64", "f64"])
def test_keys_path_and_index_path_agree(dev, name):
    """both paths against the same expected arrays, compared bit for bit: so they agree with each other"""
    udt = BY_NAME[name][3]
    for n, seed in ((1, 1), (4097, 2), (70_001, 3)):
        bits = tied_bits(udt, n, seed=seed)
        for order in (ASC, DESC):
            exp = check_unique(dev, name, bits, order, names=("counts", "offsets"), algo=-1)
            check_unique(dev, name, bits, order, names=("counts", "offsets"), algo=1, exp=exp)
            check_unique(dev, name, bits, order, names=(), algo=1, exp=exp)
    assert dev.getParam("unique.algo") == -1
    for v in (1, -1):
        dev.setParam("unique.algo", v)
        assert dev.getParam("unique.algo") == v
    for bad in (0, 2, -2):
        with pytest.raises(Exception):
            dev.setParam("unique.algo", bad)
    assert dev.getParam("unique.algo") == -1


# ---------------------------------------------------------------------------------------------
# run-length encode of grouped, unsorted keys
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint32, np.float32, np.int64, np.float64], ids=["u32", "f32", "i64", "f64"])
def test_run_length_encode_of_grouped_unsorted_keys(dev, dt):
    """A A B A: a value that comes back later starts a new run; the expected arrays come from a loop over the keys"""
    udt = np.uint32 if np.dtype(dt).itemsize == 4 else np.uint64
    rng = np.random.default_rng(44)
    pool = np.concatenate([np.frombuffer(rng.bytes(np.dtype(udt).itemsize * 5), dtype=udt), SPECIALS[np.dtype(udt).itemsize][:6]])
    lengths = rng.integers(1, 40, size=900)
    lengths[::97] = TILE[np.dtype(udt).itemsize] + 1
    picks = rng.integers(0, pool.size, size=lengths.size)
    picks[1:][picks[1:] == picks[:-1]] += 1          # adjacent runs differ
    bits = np.repeat(pool[picks % pool.size], lengths)
    keys, counts, offsets = [], [], []
    for i, b in enumerate(bits.tolist()):
        if i == 0 or b != keys[-1]:
            keys.append(b)
            counts.append(0)
            offsets.append(i)
        counts[-1] += 1
    offsets.append(bits.size)
    exp = {"unique": np.array(keys, dtype=udt), "counts": np.array(counts, np.uint32), "offsets": np.array(offsets, np.uint32)}
    assert exp["unique"].size > np.unique(bits).size, "values must come back"
    for grid in (0, 2):
        check_rle(dev, bits, grid=grid, exp=exp)
    # through the Python mirror, on the typed view of the same bits
    p = Pprims()
    buf = Buffer(dev, bits.size, dt)
    try:
        buf.write(bits.view(dt))
        res = p.runLengthEncode(dev, buf, bits.size, counts=True, offsets=True)
        r = int(res.count.toHost()[0])
        assert r == exp["unique"].size and res.firstIndex is None and res.inverse is None
        assert np.array_equal(res.unique.toHost()[:r].view(udt), exp["unique"])
        assert np.array_equal(res.counts.toHost()[:r], exp["counts"]) and np.array_equal(res.offsets.toHost()[:r + 1], exp["offsets"])
        for b in (res.unique, res.counts, res.offsets, res.count):
            b.release()
    finally:
        buf.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# the work buffer: contents on entry, size
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    n = 70_001
    bits = tied_bits(np.uint32, n, seed=31)
    other = tied_bits(np.uint32, n, seed=32, values=50)
    exp = unique_oracle(bits, "f32", DESC)
    for names in (ALL, ("counts",)):
        for fill in (0x00, 0xff):
            check_unique(dev, "f32", bits, DESC, names=names, exp=exp, fill=fill)
        # left over from a different call: other keys, other order
        w = Guarded(dev, nbytes=unique_bytes(dev, 2, n, 1), seed=9)
        try:
            check_unique(dev, "f32", other, ASC, names=names, work=w)
            check_unique(dev, "f32", bits, DESC, names=names, exp=exp, work=w)
            w.check_guard()
        finally:
            w.release()
    rexp = rle_oracle(np.sort(bits))
    for fill in (0x00, 0xff):
        check_rle(dev, np.sort(bits), exp=rexp, fill=fill)
        check_rle(dev, np.sort(bits), names=("counts",), exp=rexp, fill=fill)
    assert dev.getParam("debug.idle_dirty") == 0


def test_scratch_bytes_follow_the_documented_formulas(dev):
    """include/adlhip.h: W_runs = 16 CUs + 4 (n + 1); keys path W_runs + 2 n kb + W_keys; index path W_runs + n kb + 4 n + W_argsort;
    every part rounded up to 256 bytes"""
    lib = _lib.load()
    cus = DeviceUtils.getNCUs(dev)

    def up(x):
        return (x + 255) // 256 * 256

    def w_sort(kt, mode, m):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_sort_typed_scratch_bytes(dev._h, kt, mode, 0, m, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib_err()
        return c.value

    for name in ("f32", "i64"):
        kt, kb = BY_NAME[name][1], np.dtype(BY_NAME[name][3]).itemsize
        for n in (1, 4097, 100_003, (4 << 20) + 3):
            w_runs = up(16 * cus) + up(4 * (n + 1))
            assert rle_bytes(dev, kb, n) == w_runs
            keys_path = w_runs + 2 * up(n * kb) + up(w_sort(kt, 0, n))
            index_path = w_runs + up(n * kb) + up(4 * n) + up(w_sort(kt, 2, n))
            assert unique_bytes(dev, kt, n, 0) == keys_path
            assert unique_bytes(dev, kt, n, 1) == max(keys_path, index_path)


def test_scratch_suffices_for_smaller_inputs_and_one_byte_short_is_refused(dev):
    lib = _lib.load()
    n = 100_003
    smaller = (1, 2, 5, 4095, 4096, 4097, 16_384, 16_385, 50_000, 99_999, n)
    for name in ("f32", "i64"):
        kt, udt = BY_NAME[name][1], BY_NAME[name][3]
        for want_index in (0, 1):
            total = unique_bytes(dev, kt, n, want_index)
            for m in smaller:
                assert unique_bytes(dev, kt, m, want_index) <= total, (name, want_index, m)
            assert unique_bytes(dev, kt, n, 1) >= unique_bytes(dev, kt, n, 0)
        kb = np.dtype(udt).itemsize
        assert all(rle_bytes(dev, kb, m) <= rle_bytes(dev, kb, n) for m in smaller)
        # one buffer of the size reported for n serves the smaller inputs
        w = Guarded(dev, nbytes=unique_bytes(dev, kt, n, 1), seed=9)
        try:
            for m in (1, 4097, 50_000):
                bits = tied_bits(udt, m, seed=m)
                check_unique(dev, name, bits, ASC, work=w)
                check_unique(dev, name, bits, DESC, names=("counts",), work=w)
            w.check_guard()
        finally:
            w.release()
    # above the sizes at which the sorts change path
    for m, big in (((2 << 20) - 1, (2 << 20) + 5), ((1 << 20) + 1, (4 << 20) + 3)):
        for want_index in (0, 1):
            assert unique_bytes(dev, 2, m, want_index) <= unique_bytes(dev, 2, big, want_index)
            assert unique_bytes(dev, 5, m, want_index) <= unique_bytes(dev, 5, big, want_index)
    # one byte short
    bits = tied_bits(np.uint32, 5000, seed=3)
    inp = Guarded(dev, bits, seed=1)
    out = Outputs(dev, np.uint32, 5000, ALL)
    w = Guarded(dev, nbytes=unique_bytes(dev, 2, 5000, 1), seed=4)
    try:
        for names, want_index in ((ALL, 1), (("counts", "offsets"), 0)):
            wb = unique_bytes(dev, 2, 5000, want_index)
            args = [out.ptr(x) if x in names else None for x in ALL]
            rc = lib.adlhip_unique_typed(dev._h, 2, ASC, inp.ptr(), 5000, out.ptr("unique"), *args, out.ptr("count"), w.ptr(), wb - 1)
            assert rc == 1 and str(wb) in lib_err(), lib_err()
        wb = rle_bytes(dev, 4, 5000)
        rc = lib.adlhip_run_length_encode(dev._h, 4, inp.ptr(), 5000, out.ptr("unique"), out.ptr("counts"), out.ptr("offsets"),
                                          out.ptr("count"), w.ptr(), wb - 1)
        assert rc == 1 and str(wb) in lib_err(), lib_err()
        out.untouched()
    finally:
        for b in (inp, w):
            b.release()
        out.release()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32 = 2
    n = 5000
    bits = tied_bits(np.uint32, n, seed=71)
    inp = Guarded(dev, bits, seed=1)
    out = Outputs(dev, np.uint32, n, ALL)
    wb = unique_bytes(dev, F32, n, 1)
    w = Guarded(dev, nbytes=wb, seed=4)
    sz = ctypes.c_size_t()

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    def unique(key_type=F32, order=ASC, keys=None, m=n, u=0, c=0, o=0, f=0, i=0, cnt=0, work=0, work_bytes=wb):
        """0 = the proper buffer; anything else replaces it"""
        pick = lambda v, name: out.ptr(name) if v == 0 else v   # noqa: E731
        return lib.adlhip_unique_typed(dev._h, key_type, order, inp.ptr() if keys is None else keys, m, pick(u, "unique"), pick(c, "counts"),
                                       pick(o, "offsets"), pick(f, "first"), pick(i, "inverse"), pick(cnt, "count"),
                                       w.ptr() if work == 0 else work, work_bytes)

    def rle(key_bytes=4, keys=None, m=n, u=0, c=0, o=0, cnt=0, work=0, work_bytes=wb):
        pick = lambda v, name: out.ptr(name) if v == 0 else v   # noqa: E731
        return lib.adlhip_run_length_encode(dev._h, key_bytes, inp.ptr() if keys is None else keys, m, pick(u, "unique"), pick(c, "counts"),
                                            pick(o, "offsets"), pick(cnt, "count"), w.ptr() if work == 0 else work, work_bytes)

    def off(name, nbytes):
        return ctypes.c_void_p(out.bufs[name].buf.m_ptr + nbytes)

    try:
        for algo in (-1, 1):
            dev.setParam("unique.algo", algo)
            for fn, label in ((unique, "unique"), (rle, "run-length encode")):
                refused(fn(keys=ctypes.c_void_p(0)), label + ": NULL input")
                refused(fn(u=None), label + ": NULL d_unique_out")
                refused(fn(cnt=None), label + ": NULL count word")
                refused(fn(work=ctypes.c_void_p(0)), label + ": NULL work")
                refused(fn(keys=inp.ptr(4), m=n - 1), label + ": misaligned input")
                refused(fn(u=off("unique", 4), m=n - 1), label + ": misaligned d_unique_out")
                refused(fn(c=off("counts", 4), m=n - 1), label + ": misaligned counts")
                refused(fn(o=off("offsets", 8), m=n - 2), label + ": misaligned offsets")
                refused(fn(cnt=off("count", 2)), label + ": misaligned count word")
                refused(fn(work=w.ptr(4), work_bytes=wb - 4), label + ": misaligned work")
                refused(fn(u=inp.ptr(16)), label + ": d_unique_out overlaps the input")
                refused(fn(c=inp.ptr(n * 4 - 16)), label + ": counts overlap the input")
                refused(fn(o=inp.ptr(0)), label + ": offsets overlap the input")
                refused(fn(cnt=inp.ptr(64)), label + ": the count word overlaps the input")
                refused(fn(m=1 << 32), label + ": n = 2^32")
            refused(unique(f=off("first", 4), m=n - 1), "unique: misaligned first_index")
            refused(unique(i=off("inverse", 12), m=n - 3), "unique: misaligned inverse")
            refused(unique(f=inp.ptr(32)), "unique: first_index overlaps the input")
            refused(unique(i=inp.ptr(48)), "unique: inverse overlaps the input")
            for bad in (-1, 6, 99):
                refused(unique(key_type=bad), "key_type %d" % bad)
                refused(lib.adlhip_unique_scratch_bytes(dev._h, bad, n, 1, ctypes.byref(sz)), "scratch, key_type %d" % bad)
            for bad in (-1, 2):
                refused(unique(order=bad), "order %d" % bad)
            for bad in (0, 2, 16, -4):
                refused(rle(key_bytes=bad), "key_bytes %d" % bad)
                refused(lib.adlhip_run_length_encode_scratch_bytes(dev._h, bad, n, ctypes.byref(sz)), "scratch, key_bytes %d" % bad)
            assert str(wb) in refused(unique(work_bytes=wb - 1), "work one byte short")
            out.untouched()
            assert np.array_equal(inp.read(np.uint32), bits)
            w.check_guard()
            assert dev.getParam("debug.idle_dirty") == 0
        # n == 0 succeeds: one clear of the count word, nothing else is looked at or written
        dev.setParam("unique.algo", -1)
        assert unique(m=0) == 0, lib_err()
        got = out.bufs["count"].read(np.uint32)
        assert got[0] == 0
        out.bufs["count"].buf.write(out.sent["count"].view(np.uint8))
        assert lib.adlhip_run_length_encode(dev._h, 8, None, 0, None, None, None, out.ptr("count"), None, 0) == 0, lib_err()
        assert out.bufs["count"].read(np.uint32)[0] == 0
        out.bufs["count"].buf.write(out.sent["count"].view(np.uint8))
        out.untouched()
        refused(lib.adlhip_unique_typed(dev._h, F32, ASC, None, 0, None, None, None, None, None, None, None, 0), "n == 0 without a count word")
    finally:
        dev.setParam("unique.algo", -1)
        for b in (inp, w):
            b.release()
        out.release()


# ---------------------------------------------------------------------------------------------
# call sequences
# ---------------------------------------------------------------------------------------------
def test_call_sequences(dev):
    """unique, then a sort, then unique on one handle; the handle's device state is idle after each step"""
    n = 90_001
    a_bits = tied_bits(np.uint64, n, seed=41)
    b_bits = tied_bits(np.uint32, n, seed=42, values=37)
    keys = np.random.default_rng(43).integers(0, 1 << 32, size=n, dtype=np.uint32)
    p = Pprims()
    sort_buf = Buffer(dev, n, np.uint32)
    try:
        for algo in (-1, 1):
            check_unique(dev, "f64", a_bits, DESC, algo=algo)
            assert dev.getParam("debug.idle_dirty") == 0
            sort_buf.write(keys)
            p.radixSort(dev, sort_buf, n)
            assert np.array_equal(sort_buf.toHost(), np.sort(keys))
            assert dev.getParam("debug.idle_dirty") == 0
            check_unique(dev, "i32", b_bits, ASC, names=("counts",), algo=algo)
            assert dev.getParam("debug.idle_dirty") == 0
            check_rle(dev, np.sort(b_bits))
            assert dev.getParam("debug.idle_dirty") == 0
    finally:
        sort_buf.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# Python mirror and torch front end
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    n = 60_007
    bits = tied_bits(np.uint64, n, seed=81, values=777)
    exp = unique_oracle(bits, "f64", DESC)
    r_exp = exp["unique"].size
    p = Pprims()
    keys = Buffer(dev, n, np.float64)
    mine = Buffer(dev, n, np.uint32)
    try:
        keys.write(bits.view(np.float64))
        res = p.unique(dev, keys, n, descending=True, counts=True, offsets=True, firstIndex=True, inverse=mine)
        assert int(res.count.toHost()[0]) == r_exp and res.inverse is mine
        assert np.array_equal(res.unique.toHost()[:r_exp].view(np.uint64), exp["unique"])
        assert np.array_equal(res.counts.toHost()[:r_exp], exp["counts"]) and np.array_equal(res.offsets.toHost()[:r_exp + 1], exp["offsets"])
        assert np.array_equal(res.firstIndex.toHost()[:r_exp], exp["first"]) and np.array_equal(mine.toHost(), exp["inverse"])
        assert np.array_equal(keys.toHost().view(np.uint64), bits)
        for b in (res.unique, res.counts, res.offsets, res.firstIndex, res.count):
            b.release()
        res = p.unique(dev, keys, n)
        assert res.counts is None and res.offsets is None and res.firstIndex is None and res.inverse is None
        assert int(res.count.toHost()[0]) == np.unique(bits).size
        for b in (res.unique, res.count):
            b.release()
        res = p.unique(dev, keys, 0, counts=True)
        assert int(res.count.toHost()[0]) == 0
        for b in (res.unique, res.counts, res.count):
            b.release()
    finally:
        keys.release()
        mine.release()
        p.close()


@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(torch, dtype, shape, seed=11):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-300, 300, shape, dtype=torch.int64, device="cuda", generator=g)   # many ties
    if dtype.is_floating_point:
        t = torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25   # no -0 (and no +0 either), no NaN
    return t.to(dtype)


@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_unique_matches_torch(sorter, dtype_name):
    import torch
    dtype = getattr(torch, dtype_name)
    t = _torch_input(torch, dtype, (100_003,))
    keep = t.clone()
    for inputs in (t, _torch_input(torch, dtype, (37, 5, 101), seed=12), t[::2], _torch_input(torch, dtype, (64, 66), seed=13)[:, 1:65],
                   t[1:]):
        want = torch.unique(inputs, sorted=True, return_inverse=True, return_counts=True)
        got = sorter.unique(inputs, return_inverse=True, return_counts=True)
        torch.cuda.synchronize()
        assert len(got) == 3
        for g, w_ in zip(got, want):
            assert g.dtype == w_.dtype and g.shape == w_.shape and torch.equal(g, w_)
        assert got[1].shape == inputs.shape and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
        u = sorter.unique(inputs)
        assert isinstance(u, torch.Tensor) and torch.equal(u, want[0])
        u, c = sorter.unique(inputs, return_counts=True)
        assert torch.equal(u, want[0]) and torch.equal(c, want[2])
        u, inv = sorter.unique(inputs, return_inverse=True)
        assert torch.equal(u, want[0]) and torch.equal(inv, want[1])
    assert not t[::2].is_contiguous()
    assert torch.equal(t, keep), "the input was changed"
    empty = torch.empty((0, 3), dtype=dtype, device="cuda")
    u, inv, c = sorter.unique(empty, return_inverse=True, return_counts=True)
    assert u.numel() == 0 and u.dtype == dtype and inv.shape == (0, 3) and inv.dtype == torch.int64 and c.numel() == 0 and c.dtype == torch.int64


@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_unique_consecutive_matches_torch(sorter, dtype_name):
    import torch
    dtype = getattr(torch, dtype_name)
    g = torch.Generator(device="cuda").manual_seed(14)
    lengths = torch.randint(1, 9, (20_000,), device="cuda", generator=g)
    t = torch.repeat_interleave(_torch_input(torch, dtype, (20_000,), seed=15), lengths)   # grouped, not sorted: values come back
    keep = t.clone()
    for inputs in (t, t[::2], t[1:]):
        want_u, want_c = torch.unique_consecutive(inputs, return_counts=True)
        u, c = sorter.unique_consecutive(inputs, return_counts=True)
        assert u.dtype == dtype and c.dtype == torch.int64 and torch.equal(u, want_u) and torch.equal(c, want_c)
        u = sorter.unique_consecutive(inputs)
        assert isinstance(u, torch.Tensor) and torch.equal(u, want_u)
    assert torch.equal(t, keep), "the input was changed"
    u, c = sorter.unique_consecutive(torch.empty(0, dtype=dtype, device="cuda"), return_counts=True)
    assert u.numel() == 0 and c.numel() == 0 and c.dtype == torch.int64
    with pytest.raises(ValueError):
        sorter.unique_consecutive(torch.zeros((4, 4), dtype=dtype, device="cuda"))


def test_torch_sorter_unique_is_bound_to_its_stream(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.tensor([3, 1, 3, 2, 1, 3], dtype=torch.int32, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "unique", boom)
        monkeypatch.setattr(sorter.pprims, "runLengthEncode", boom)
        with pytest.raises(RuntimeError):
            sorter.unique(t)
        with pytest.raises(RuntimeError):
            sorter.unique_consecutive(t)
        monkeypatch.undo()
    u, inv, c = sorter.unique(t, return_inverse=True, return_counts=True)
    assert u.tolist() == [1, 2, 3] and inv.tolist() == [2, 0, 2, 1, 0, 2] and c.tolist() == [2, 1, 3]
    u, c = sorter.unique_consecutive(t, return_counts=True)
    assert u.tolist() == [3, 1, 3, 2, 1, 3] and c.tolist() == [1] * 6
    for bad in (torch.zeros(8, dtype=torch.float16, device="cuda"), torch.zeros(8, dtype=torch.float32), [3.0, 1.0]):
        with pytest.raises((TypeError, ValueError)):
            sorter.unique(bad)
        with pytest.raises((TypeError, ValueError)):
            sorter.unique_consecutive(bad)
