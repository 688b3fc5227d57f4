"""Reduce values by key on the GPU (include/adlhip.h "reduce values by key"; oclradixsort_amd/csrc/reduce_kernels.hpp;
Pprims.reduceByKey / reduceRuns; TorchSorter.reduce_by_key / reduce_consecutive).

The oracle is numpy: run heads from the key bits, then np.add.reduceat (integer sums on the unsigned view, which wrap; float sums on
the typed view) and np.minimum.reduceat / np.maximum.reduceat on the order-preserving code of the VALUES (the code of include/adlhip.h
"typed keys", ascending).  reduce_by_key goes through the stable argsort of the keys' code first.  tests/test_reduce_api.py checks the
oracle against a plain loop on the CPU.

Everything structural is compared bit for bit: integer sums, min and max always; float sums on values that are small integers stored
as floats, whose sums are exact in every association.  One case per float type uses random values and the textbook bound for any
summation order.

Every output is prefilled with sentinels and read back whole: the first R elements (offsets: R + 1) must be the expected ones,
everything behind them the sentinels.  Every device buffer carries guard bytes behind its payload -- both inputs, every output (sized
exactly n, offsets n + 1), the count word and the work buffer (sized exactly the reported bytes) -- and the inputs are compared with
their originals afterwards.

T below is the tile of the reduce stage, 2048 elements whatever the widths (reduce_kernels.hpp: kRedTile); PER = the elements of one
16-byte vector of the narrower of the two arrays.
"""
import ctypes
import math

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib

pytestmark = pytest.mark.gpu

ASC, DESC = 0, 1
SUM, MIN, MAX = 0, 1, 2
OPS = (SUM, MIN, MAX)
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max"}
TYPES = [("u32", 0, np.uint32, np.uint32), ("i32", 1, np.int32, np.uint32), ("f32", 2, np.float32, np.uint32),
         ("u64", 3, np.uint64, np.uint64), ("i64", 4, np.int64, np.uint64), ("f64", 5, np.float64, np.uint64)]
BY_NAME = {t[0]: t for t in TYPES}
TYPE_IDS = [t[0] for t in TYPES]
SENTINELS = 64
T = 2048
N40 = 40 * T + 3

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


def per(kw, vw):
    return 16 // min(kw, vw)


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def encode(bits, name, order=ASC):
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


def decode(code, name):
    """the inverse of encode(.., ASC)"""
    w = code.dtype.itemsize
    udt = code.dtype.type
    sign = udt(1 << (8 * w - 1))
    if name[0] == "i":
        return code ^ sign
    if name[0] == "f":
        return np.where(code & sign != 0, code ^ sign, ~code).astype(udt)
    return code.copy()


def runs_oracle(kbits, vbits, vname, op):
    """the runs of kbits (grouped) and op over the values of each; vbits are bit patterns of type vname"""
    heads = np.flatnonzero(np.concatenate([[True], kbits[1:] != kbits[:-1]]))
    offsets = np.concatenate([heads, [kbits.size]]).astype(np.uint32)
    if op == SUM and vname[0] == "f":
        with np.errstate(all="ignore"):
            red = np.add.reduceat(vbits.view(BY_NAME[vname][2]), heads).view(vbits.dtype)
    elif op == SUM:
        red = np.add.reduceat(vbits, heads)          # unsigned: wraps, the same bits as the signed sum
    else:
        code = encode(vbits, vname)
        red = decode((np.minimum if op == MIN else np.maximum).reduceat(code, heads), vname)
    return {"unique": kbits[heads], "offsets": offsets, "counts": np.diff(offsets).astype(np.uint32), "reduced": red.astype(vbits.dtype)}


def by_key_oracle(kbits, kname, order, vbits, vname, op):
    perm = np.argsort(encode(kbits, kname, order), kind="stable")
    return runs_oracle(kbits[perm], vbits[perm], vname, op)


def random_bits(udt, n, rng, specials=True):
    w = np.dtype(udt).itemsize
    v = np.frombuffer(rng.bytes(w * max(n, 1)), dtype=udt)[:n].copy()
    if specials and n >= 64:
        where = rng.integers(0, n, size=SPECIALS[w].size * 3)
        v[where] = np.tile(SPECIALS[w], 3)
    return v


def values_for(vname, op, n, rng):
    """bit patterns of type vname on which op is exact: anything for integer sums (they wrap) and for min / max (special patterns
    included); small integers stored as floats for float sums (|sum| <= 8 n < 2^24 for every n used here)"""
    udt = BY_NAME[vname][3]
    if op == SUM and vname[0] == "f":
        assert 8 * n < 1 << 24
        return rng.integers(-8, 9, size=n).astype(BY_NAME[vname][2]).view(udt)
    v = random_bits(udt, n, rng)
    if op == SUM and n >= 8:   # values near the type's limits, so that wraps occur at once
        v[::3] = udt((1 << (8 * v.dtype.itemsize - 1)) - 1)
    return v


def keys_from_lengths(udt, lengths, rng, sort=True):
    """grouped keys with the given run lengths: distinct random bit patterns (ascending when sort)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    w = np.dtype(udt).itemsize
    pool = np.unique(np.frombuffer(rng.bytes(w * (lengths.size * 2 + 8)), dtype=udt))[:lengths.size]
    assert pool.size == lengths.size
    if not sort:
        pool = pool[rng.permutation(pool.size)]
    return np.repeat(pool, lengths)


def sentinels(dtype, count, salt):
    return (np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ np.uint64(salt)).astype(dtype)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.reduce_grid", 0)
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


def runs_bytes(dev, kb, vt, n):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_reduce_runs_scratch_bytes(dev._h, kb, vt, n, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def by_key_bytes(dev, kt, vt, n):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_reduce_by_key_scratch_bytes(dev._h, kt, vt, n, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Outputs:
    """sentinel-filled outputs of one call: unique, reduced and the count word always, counts / offsets where named"""

    EXTRA = {"offsets": 1}   # elements beyond n

    def __init__(self, dev, kudt, vudt, n, names=("counts", "offsets")):
        self.n = n
        self.sent = {"unique": sentinels(kudt, n, 0xa5a5a5a5a5a5a5a5), "reduced": sentinels(vudt, n, 0x3c3c3c3c3c3c3c3c),
                     "count": np.array([0xdeadbeef], np.uint32)}
        for i, name in enumerate(names):
            self.sent[name] = sentinels(np.uint32, n + self.EXTRA.get(name, 0), 0x5a5a5a5a + i)
        self.bufs = {}
        for i, (name, s) in enumerate(self.sent.items()):
            self.bufs[name] = Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=10 + i)

    def ptr(self, name):
        return self.bufs[name].ptr() if name in self.bufs else None

    def check(self, exp, what):
        got = {name: b.read(self.sent[name].dtype) for name, b in self.bufs.items()}
        r = int(got["count"][0])
        assert r == exp["unique"].size, "%s: %d runs, expected %d" % (what, r, exp["unique"].size)
        for name, g in got.items():
            if name == "count":
                continue
            m = r + self.EXTRA.get(name, 0)
            if not np.array_equal(g[:m], exp[name]):
                bad = np.flatnonzero(g[:m] != exp[name])
                raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                    what, name, bad.size, m, bad[0], int(g[bad[0]]), int(exp[name][bad[0]])))
            assert np.array_equal(g[m:], self.sent[name][m:]), "%s: %s was written at index %d or beyond" % (what, name, m)
        return got["reduced"][:r].copy() if "reduced" in got else None

    def untouched(self):
        for name, b in self.bufs.items():
            assert np.array_equal(b.read(self.sent[name].dtype), self.sent[name]), "%s was written" % name

    def release(self):
        for b in self.bufs.values():
            b.release()


def run_reduce(dev, kbits, vname, vbits, op, by_key=None, names=("counts", "offsets"), grid=0, exp=None, work=None, fill=None):
    """one call of adlhip_reduce_runs (by_key None) or adlhip_reduce_by_key_typed (by_key = (key type name, order)) with every check of
    the memory contract; exp: the expected arrays, or a function of the structural oracle's result that returns them (float sums that
    are not exact: `reduced` is then checked by the caller).  Returns (exp, reduced as read back)."""
    n, kb = kbits.size, kbits.dtype.itemsize
    vt, vudt = BY_NAME[vname][1], BY_NAME[vname][3]
    assert vbits.dtype == vudt and vbits.size == n
    if exp is None:
        exp = by_key_oracle(kbits, by_key[0], by_key[1], vbits, vname, op) if by_key else runs_oracle(kbits, vbits, vname, op)
    check_reduced = exp.get("reduced") is not None
    dev.setParam("debug.reduce_grid", grid)
    wb = by_key_bytes(dev, BY_NAME[by_key[0]][1], vt, n) if by_key else runs_bytes(dev, kb, vt, n)
    kin = Guarded(dev, kbits, guard_bytes=SENTINELS * kb, seed=5)
    vin = Guarded(dev, vbits, guard_bytes=SENTINELS * vbits.dtype.itemsize, seed=6)
    out = Outputs(dev, kbits.dtype.type, vudt, n, names)
    own = work is None
    w = Guarded(dev, nbytes=wb, seed=8, fill=fill) if own else work
    what = "%s keys %s, %s of %s, n %d grid %d" % ("by key %s order %d" % by_key if by_key else "runs", kbits.dtype, OP_NAMES[op], vname, n, grid)
    lib = _lib.load()
    try:
        if by_key:
            rc = lib.adlhip_reduce_by_key_typed(dev._h, BY_NAME[by_key[0]][1], by_key[1], kin.ptr(), vt, op, vin.ptr(), n, out.ptr("unique"),
                                                out.ptr("reduced"), out.ptr("counts"), out.ptr("offsets"), out.ptr("count"), w.ptr(), w.nbytes)
        else:
            rc = lib.adlhip_reduce_runs(dev._h, kb, kin.ptr(), vt, op, vin.ptr(), n, out.ptr("unique"), out.ptr("reduced"), out.ptr("counts"),
                                        out.ptr("offsets"), out.ptr("count"), w.ptr(), w.nbytes)
        assert rc == 0, lib_err()
        if check_reduced:
            got = out.check(exp, what)
        else:   # the structure here, the sums by the caller; behind R the sentinels all the same
            r = exp["unique"].size
            raw = out.bufs["reduced"].read(vudt)
            assert np.array_equal(raw[r:], out.sent["reduced"][r:]), what + ": reduced was written at index R or beyond"
            got = raw[:r].copy()
            out.bufs.pop("reduced").release()
            out.check({k: v for k, v in exp.items() if k != "reduced"}, what)
        w.check_guard()
        assert np.array_equal(kin.read(kbits.dtype), kbits), what + ": d_keys_in was changed"
        assert np.array_equal(vin.read(vbits.dtype), vbits), what + ": d_vals_in was changed"
    finally:
        dev.setParam("debug.reduce_grid", 0)
        kin.release()
        vin.release()
        out.release()
        if own:
            w.release()
    return exp, got


# ---------------------------------------------------------------------------------------------
# every (key width, value type, op); every key type and order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", TYPE_IDS)
@pytest.mark.parametrize("kw", [4, 8], ids=["k32", "k64"])
def test_every_key_width_value_type_and_op(dev, kw, vname):
    n = 3 * T + 5
    rng = np.random.default_rng(100 + kw + BY_NAME[vname][1])
    lengths = rng.integers(1, 40, size=n)
    lengths = lengths[:np.searchsorted(np.cumsum(lengths), n)]
    lengths = np.concatenate([lengths, [n - lengths.sum()]])
    kbits = keys_from_lengths(np.uint32 if kw == 4 else np.uint64, lengths, rng, sort=False)
    for op in OPS:
        vbits = values_for(vname, op, n, rng)
        run_reduce(dev, kbits, vname, vbits, op)
        run_reduce(dev, kbits, vname, vbits, op, names=("counts",))      # the offsets live in the work buffer
        run_reduce(dev, kbits, vname, vbits, op, names=())
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_reduce_by_key_every_key_type_and_order_with_special_patterns(dev, kname, order):
    n = 3 * T + 5
    kudt = BY_NAME[kname][3]
    rng = np.random.default_rng(200 + BY_NAME[kname][1])
    pool = np.concatenate([np.frombuffer(rng.bytes(np.dtype(kudt).itemsize * 300), dtype=kudt), SPECIALS[np.dtype(kudt).itemsize]])
    kbits = np.ascontiguousarray(pool[rng.integers(0, pool.size, size=n)])
    assert np.isin(SPECIALS[np.dtype(kudt).itemsize], kbits).all()
    for vname, op in (("f32", SUM), ("i64", SUM), ("f64", MIN), ("i32", MAX), ("f32", MAX), ("u64", MIN)):
        run_reduce(dev, kbits, vname, values_for(vname, op, n, rng), op, by_key=(kname, order))
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# sizes: vector, tile and chunk edges
# ---------------------------------------------------------------------------------------------
_SIZE_COMBOS = [("u32", "f32"), ("f64", "i64"), ("i32", "f64")]
_SIZE_CASES = sorted(set((k, v, n) for k, v in _SIZE_COMBOS
                         for p in [per(np.dtype(BY_NAME[k][3]).itemsize, np.dtype(BY_NAME[v][3]).itemsize)]
                         for n in (0, 1, 2, p - 1, p, p + 1, T - 1, T, T + 1, 2 * T + 3, N40)))


@pytest.mark.parametrize("kname,vname,n", _SIZE_CASES, ids=["%s-%s-%d" % c for c in _SIZE_CASES])
def test_sizes(dev, kname, vname, n):
    rng = np.random.default_rng(7 * n + 1)
    kudt = BY_NAME[kname][3]
    pool = np.frombuffer(rng.bytes(np.dtype(kudt).itemsize * max(1, n // 3)), dtype=kudt)
    kbits = np.ascontiguousarray(pool[rng.integers(0, pool.size, size=n)])
    if n == 0:
        lib = _lib.load()
        cnt = Guarded(dev, np.array([0xdeadbeef], np.uint32), seed=3)
        try:
            vt = BY_NAME[vname][1]
            assert lib.adlhip_reduce_runs(dev._h, kbits.dtype.itemsize, None, vt, SUM, None, 0, None, None, None, None, cnt.ptr(), None, 0) == 0, lib_err()
            assert cnt.read(np.uint32)[0] == 0
            cnt.buf.write(np.array([0xdeadbeef], np.uint32).view(np.uint8))
            assert lib.adlhip_reduce_by_key_typed(dev._h, BY_NAME[kname][1], DESC, None, vt, MAX, None, 0, None, None, None, None, cnt.ptr(),
                                                  None, 0) == 0, lib_err()
            assert cnt.read(np.uint32)[0] == 0
            assert lib.adlhip_reduce_runs(dev._h, 4, None, vt, SUM, None, 0, None, None, None, None, None, None, 0) == 1
        finally:
            cnt.release()
        return
    for op in OPS:
        vbits = values_for(vname, op, n, rng)
        run_reduce(dev, np.sort(kbits), vname, vbits, op)
        run_reduce(dev, kbits, vname, vbits, op, by_key=(kname, ASC if op != MIN else DESC))
    assert dev.getParam("debug.idle_dirty") == 0


def test_one_large_size(dev):
    n = (1 << 20) + 3
    rng = np.random.default_rng(5)
    kbits = rng.integers(0, 5000, size=n).astype(np.uint32)
    vbits = values_for("f32", SUM, n, rng)
    run_reduce(dev, kbits, "f32", vbits, SUM, by_key=("u32", ASC))
    run_reduce(dev, np.sort(kbits).astype(np.uint64), "i64", values_for("i64", MIN, n, rng), MIN)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# run shapes x grids x widths
# ---------------------------------------------------------------------------------------------
def _run_shapes():
    """run lengths that sum to N40 = 40 T + 3.  "debug.reduce_grid" 0 gives one tile per chunk, 1 one chunk, 3 chunks of 14 tiles."""
    c = 14 * T

    def pad(lengths):
        rest = N40 - sum(lengths)
        assert rest > 0
        return lengths + [rest]

    return {
        "all-equal": [N40],                                              # the carry crosses every chunk, no chunk but the first has a head
        "all-distinct": [1] * N40,
        "one-run-per-tile": [T] * 40 + [3],
        "ends-on-tile-and-chunk-ends": pad([T, 5, T - 5, c - 2 * T, 7, T - 7, c - T, T - 1, 1]),
        "starts-at-second-element-of-chunk": pad([T + 1, T, c - 2 * T, c]),
        "whole-chunks-then-mid-chunk": pad([3, 30 * T + 100]),           # grid 3: covers chunk 1 whole, ends inside chunk 2
        "alternating-1-and-3T": pad([1, 3 * T] * 13),
        "last-run-of-one": [N40 - 1 - 5 * T, 5 * T, 1],
        "tiles-without-a-head": pad([1, 3 * T + T // 2, 2, 1, 5, T // 3, 6 * T + 1, 17]),
    }


_WIDTHS = [(4, "f32"), (4, "i64"), (8, "f32"), (8, "f64"), (4, "f64"), (8, "i32")]
_SHAPES = [(s, kw, v) for s in _run_shapes() for kw, v in _WIDTHS]


@pytest.mark.parametrize("shape,kw,vname", _SHAPES, ids=["%s-k%d-%s" % (s, 8 * kw, v) for s, kw, v in _SHAPES])
def test_run_shapes_grids_and_mixed_widths(dev, shape, kw, vname):
    lengths = _run_shapes()[shape]
    assert sum(lengths) == N40
    rng = np.random.default_rng(22)
    kbits = keys_from_lengths(np.uint32 if kw == 4 else np.uint64, lengths, rng)
    for op in OPS:
        vbits = values_for(vname, op, N40, rng)
        exp, first = run_reduce(dev, kbits, vname, vbits, op, grid=0)
        assert np.array_equal(exp["counts"].astype(np.int64), np.asarray(lengths))
        for grid in (1, 3):
            _, got = run_reduce(dev, kbits, vname, vbits, op, grid=grid, exp=exp)
            assert np.array_equal(got, first), "the result depends on the grid"
    assert dev.getParam("debug.idle_dirty") == 0


def test_reduce_grid_knob(dev):
    assert dev.getParam("debug.reduce_grid") == 0
    dev.setParam("debug.reduce_grid", 3)
    assert dev.getParam("debug.reduce_grid") == 3
    dev.setParam("debug.reduce_grid", 0)
    with pytest.raises(Exception):
        dev.setParam("debug.reduce_grid", -1)
    # larger than the default grid: changes nothing
    rng = np.random.default_rng(3)
    kbits = np.sort(rng.integers(0, 900, size=N40).astype(np.uint32))
    vbits = values_for("f32", SUM, N40, rng)
    exp, a = run_reduce(dev, kbits, "f32", vbits, SUM)
    _, b = run_reduce(dev, kbits, "f32", vbits, SUM, grid=1 << 20, exp=exp)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# float sums: the one tolerance case, determinism, single elements, propagation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_sums_of_random_values_within_the_bound_of_any_order_and_deterministic(dev, vname):
    """|s^ - s| <= gamma_(m-1) sum|x_i| + u |s|, gamma_k = k u / (1 - k u): the bound of ANY summation order of m numbers (Higham,
    Accuracy and Stability of Numerical Algorithms, section 4.2), plus the rounding of the exact sum itself.  s: math.fsum per run
    (f64), float64 numpy (f32)."""
    n = 64 * T + 1
    dt, udt = BY_NAME[vname][2], BY_NAME[vname][3]
    u = 2.0 ** -24 if vname == "f32" else 2.0 ** -53
    rng = np.random.default_rng(77)
    lengths = np.concatenate([rng.integers(1, 6, size=20000), rng.integers(50, 400, size=200), [3 * T + 7, T, 9 * T + 1]])
    lengths = lengths[rng.permutation(lengths.size)]
    lengths = lengths[:np.searchsorted(np.cumsum(lengths), n)]
    lengths = np.concatenate([lengths, [n - lengths.sum()]])
    kbits = keys_from_lengths(np.uint64, lengths, rng, sort=False)
    vals = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, size=n))).astype(dt)
    vbits = vals.view(udt)
    structure = runs_oracle(kbits, vbits, vname, SUM)
    structure["reduced"] = None
    seen = []
    for fill in (None, 0x00, 0xff, None):     # twice on scratch as it comes, and on two fresh work buffers with different fill
        _, got = run_reduce(dev, kbits, vname, vbits, SUM, exp=structure, fill=fill)
        seen.append(got)
    for g in seen[1:]:
        assert np.array_equal(g, seen[0]), "the same call gave other bits"
    got = seen[0].view(dt).astype(np.float64)
    off = structure["offsets"].astype(np.int64)
    x = vals.astype(np.float64)
    worst = 0.0
    for r in range(off.size - 1):
        seg = x[off[r]:off[r + 1]]
        m = seg.size
        s = math.fsum(seg.tolist()) if vname == "f64" else float(seg.sum())
        k = m - 1
        bound = (k * u / (1 - k * u)) * float(np.abs(seg).sum()) + u * abs(s)
        err = abs(float(got[r]) - s)
        worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
        assert err <= bound, "run %d of %d elements: |%r - %r| = %g > %g" % (r, m, got[r], s, err, bound)
    print("largest error / bound: %.3f" % worst)
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("vname", TYPE_IDS)
def test_single_element_runs_return_the_element_bit_for_bit(dev, vname):
    n = 3 * T + 5
    vudt = BY_NAME[vname][3]
    rng = np.random.default_rng(9)
    sp = SPECIALS[np.dtype(vudt).itemsize]
    vbits = np.ascontiguousarray(np.tile(sp, n // sp.size + 1)[:n])
    kbits = np.arange(n, dtype=np.uint32) * np.uint32(7)
    for op in OPS:
        for grid in (0, 2):
            exp, got = run_reduce(dev, kbits, vname, vbits, op, grid=grid, exp={**runs_oracle(kbits, vbits, vname, MAX), "reduced": vbits})
            assert np.array_equal(got, vbits)
    # and through the sort: shuffled distinct keys
    perm = rng.permutation(n)
    for op in OPS:
        run_reduce(dev, kbits[perm].astype(np.uint64), vname, vbits[perm], op, by_key=("u64", ASC),
                   exp={**runs_oracle(kbits.astype(np.uint64), vbits, vname, MAX), "reduced": vbits})
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_propagation(dev, vname):
    dt, udt = BY_NAME[vname][2], BY_NAME[vname][3]
    nan, inf, nz = np.nan, np.inf, -0.0
    runs = [("nan", [1.0, 2.0, nan, 3.0] + [1.0] * 300), ("nan", [nan] + [2.0] * (T + 3)), ("nan", [inf, 1.0, -inf] + [0.5] * 70),
            ("nan", [1.0] * (2 * T) + [-inf, 4.0, inf]), ("+inf", [inf, 1.0, inf] + [-3.0] * 40), ("-inf", [-inf] + [7.0] * (T - 1)),
            ("-0", [nz] * 2), ("-0", [nz] * (3 * T + 1)), ("-0", [nz]), ("+0", [nz, 0.0, nz]), ("+0", [1.0, -1.0]), ("nan", [nan, nan])]
    vals = np.concatenate([np.array(r, dtype=dt) for _, r in runs])
    kbits = np.repeat(np.arange(len(runs), dtype=np.uint32)[::-1].copy(), [len(r) for _, r in runs])
    vbits = np.ascontiguousarray(vals).view(udt)
    structure = runs_oracle(kbits, vbits, vname, SUM)
    structure["reduced"] = None
    for grid in (0, 1, 3):
        _, got = run_reduce(dev, kbits, vname, vbits, SUM, exp=structure, grid=grid)
        got = got.view(dt)
        for (cls, _), g in zip(runs, got):
            if cls == "nan":
                assert np.isnan(g)
            elif cls in ("+inf", "-inf"):
                assert np.isinf(g) and (g > 0) == (cls == "+inf")
            else:
                assert g == 0 and bool(np.signbit(g)) == (cls == "-0"), "expected %s, got %r" % (cls, g)
        for op in (MIN, MAX):
            run_reduce(dev, kbits, vname, vbits, op, grid=grid)     # the totalOrder oracle
    # what totalOrder means here: NaN with the sign bit clear is the largest, -0 is below +0
    exp = runs_oracle(kbits, vbits, vname, MAX)
    assert np.isnan(exp["reduced"].view(dt)[0]) and np.isnan(exp["reduced"].view(dt)[1]) and exp["reduced"].view(dt)[2] == np.inf
    lo = runs_oracle(kbits, vbits, vname, MIN)["reduced"].view(dt)
    assert lo[2] == -np.inf and lo[9] == 0 and np.signbit(lo[9])
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# grouped but unsorted keys; the two-way check against unique
# ---------------------------------------------------------------------------------------------
def test_reduce_runs_on_grouped_unsorted_keys(dev):
    """A A B A: three runs; the expected arrays come from a loop"""
    a, b = 0x7fc00123, 5
    kbits = np.array([a, a, b, a], dtype=np.uint32)
    vals = np.array([10, 20, 30, 40], dtype=np.int32)
    exp = {"unique": np.array([a, b, a], np.uint32), "counts": np.array([2, 1, 1], np.uint32), "offsets": np.array([0, 2, 3, 4], np.uint32)}
    for op, red in ((SUM, [30, 30, 40]), (MIN, [10, 30, 40]), (MAX, [20, 30, 40])):
        run_reduce(dev, kbits, "i32", vals.view(np.uint32), op, exp={**exp, "reduced": np.array(red, np.int32).view(np.uint32)})
    # longer: values come back, runs across tiles
    rng = np.random.default_rng(44)
    pool = np.concatenate([np.frombuffer(rng.bytes(8 * 5), dtype=np.uint64), SPECIALS[8][:6]])
    lengths = rng.integers(1, 40, size=900)
    lengths[::97] = T + 1
    picks = rng.integers(0, pool.size, size=lengths.size)
    picks[1:][picks[1:] == picks[:-1]] += 1          # adjacent runs differ
    kbits = np.repeat(pool[picks % pool.size], lengths)
    keys, red, counts = [], [], []
    vals = rng.integers(-1000, 1000, size=kbits.size).astype(np.int64)
    for k, v in zip(kbits.tolist(), vals.tolist()):
        if not keys or k != keys[-1]:
            keys.append(k)
            red.append(0)
            counts.append(0)
        red[-1] += v
        counts[-1] += 1
    assert len(keys) > np.unique(kbits).size, "values must come back"
    exp = {"unique": np.array(keys, np.uint64), "counts": np.array(counts, np.uint32),
           "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), "reduced": np.array(red, np.int64).view(np.uint64)}
    for grid in (0, 2):
        run_reduce(dev, kbits, "i64", vals.view(np.uint64), SUM, grid=grid, exp=exp)


@pytest.mark.parametrize("kname,vname", [("f32", "i64"), ("i64", "f32"), ("u32", "u32"), ("f64", "f64")])
def test_reduce_by_key_against_the_oracle_and_against_unique(dev, kname, vname):
    n = 70_001
    lib = _lib.load()
    kt, kudt = BY_NAME[kname][1], BY_NAME[kname][3]
    rng = np.random.default_rng(61)
    pool = np.concatenate([np.frombuffer(rng.bytes(np.dtype(kudt).itemsize * 2000), dtype=kudt), SPECIALS[np.dtype(kudt).itemsize]])
    kbits = np.ascontiguousarray(pool[rng.integers(0, pool.size, size=n)])
    for order in (ASC, DESC):
        # what adlhip_unique_typed gives for the same keys
        wb = ctypes.c_size_t()
        assert lib.adlhip_unique_scratch_bytes(dev._h, kt, n, 0, ctypes.byref(wb)) == 0, lib_err()
        kin = Guarded(dev, kbits, seed=1)
        w = Guarded(dev, nbytes=wb.value, seed=2)
        uo = Outputs(dev, kudt, np.uint32, n)
        try:
            rc = lib.adlhip_unique_typed(dev._h, kt, order, kin.ptr(), n, uo.ptr("unique"), uo.ptr("counts"), uo.ptr("offsets"), None, None,
                                         uo.ptr("count"), w.ptr(), w.nbytes)
            assert rc == 0, lib_err()
            r = int(uo.bufs["count"].read(np.uint32)[0])
            from_unique = {"unique": uo.bufs["unique"].read(kudt)[:r].copy(), "counts": uo.bufs["counts"].read(np.uint32)[:r].copy(),
                           "offsets": uo.bufs["offsets"].read(np.uint32)[:r + 1].copy()}
        finally:
            for b in (kin, w):
                b.release()
            uo.release()
        for op in OPS:
            vbits = values_for(vname, op, n, rng)
            exp = by_key_oracle(kbits, kname, order, vbits, vname, op)
            for name, arr in from_unique.items():
                assert np.array_equal(arr, exp[name]), name
            run_reduce(dev, kbits, vname, vbits, op, by_key=(kname, order), exp={**from_unique, "reduced": exp["reduced"]})
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# the work buffer: contents on entry, size
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    n = 70_001
    rng = np.random.default_rng(31)
    kbits = rng.integers(0, 3000, size=n).astype(np.uint32)
    other = rng.integers(0, 50, size=n).astype(np.uint32)
    for vname, op in (("f32", SUM), ("i64", MIN)):
        vbits = values_for(vname, op, n, rng)
        vt = BY_NAME[vname][1]
        exp = by_key_oracle(kbits, "i32", DESC, vbits, vname, op)
        rexp = runs_oracle(np.sort(kbits), vbits, vname, op)
        for fill in (0x00, 0xff):
            run_reduce(dev, kbits, vname, vbits, op, by_key=("i32", DESC), exp=exp, fill=fill)
            run_reduce(dev, np.sort(kbits), vname, vbits, op, exp=rexp, fill=fill)
            run_reduce(dev, np.sort(kbits), vname, vbits, op, names=("counts",), exp=rexp, fill=fill)
        # left over from a different call: other keys, other order, other operator
        w = Guarded(dev, nbytes=by_key_bytes(dev, 1, vt, n), seed=9)
        try:
            run_reduce(dev, other, vname, values_for(vname, MAX, n, rng), MAX, by_key=("i32", ASC), work=w)
            run_reduce(dev, kbits, vname, vbits, op, by_key=("i32", DESC), exp=exp, work=w)
            w.check_guard()
        finally:
            w.release()
    assert dev.getParam("debug.idle_dirty") == 0


def test_scratch_bytes_follow_the_documented_formulas(dev):
    """include/adlhip.h: W_reduce = 16 CUs + 16 CUs + 32 CUs + 32 CUs + 4 (n + 1); by key: W_reduce + n kb + n vb + W_argsort; every part
    rounded up to 256 bytes"""
    lib = _lib.load()
    cus = DeviceUtils.getNCUs(dev)

    def up(x):
        return (x + 255) // 256 * 256

    def w_argsort(kt, m):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_sort_typed_scratch_bytes(dev._h, kt, 2, 0, m, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib_err()
        return c.value

    for kname in ("f32", "i64"):
        for vname in ("i32", "f64"):
            kt, kb = BY_NAME[kname][1], np.dtype(BY_NAME[kname][3]).itemsize
            vt, vb = BY_NAME[vname][1], np.dtype(BY_NAME[vname][3]).itemsize
            for n in (1, 4097, 100_003, (4 << 20) + 3):
                w_reduce = 2 * up(16 * cus) + 2 * up(32 * cus) + up(4 * (n + 1))
                assert runs_bytes(dev, kb, vt, n) == w_reduce
                assert by_key_bytes(dev, kt, vt, n) == w_reduce + up(n * kb) + up(n * vb) + up(w_argsort(kt, n))


def test_scratch_suffices_for_smaller_inputs_and_one_byte_short_is_refused(dev):
    lib = _lib.load()
    n = 100_003
    smaller = (1, 2, 5, 2047, 2048, 2049, 16_384, 16_385, 50_000, 99_999, n)
    rng = np.random.default_rng(8)
    for kname, vname in (("f32", "f64"), ("i64", "i32")):
        kt, kudt = BY_NAME[kname][1], BY_NAME[kname][3]
        vt = BY_NAME[vname][1]
        kb = np.dtype(kudt).itemsize
        total = by_key_bytes(dev, kt, vt, n)
        assert all(by_key_bytes(dev, kt, vt, m) <= total for m in smaller)
        assert all(runs_bytes(dev, kb, vt, m) <= runs_bytes(dev, kb, vt, n) for m in smaller)
        w = Guarded(dev, nbytes=total, seed=9)      # one buffer of the size reported for n serves the smaller inputs
        try:
            for m in (1, 2049, 50_000):
                kbits = rng.integers(0, max(1, m // 7), size=m).astype(kudt)
                run_reduce(dev, kbits, vname, values_for(vname, SUM, m, rng), SUM, by_key=(kname, ASC), work=w)
                run_reduce(dev, kbits, vname, values_for(vname, MAX, m, rng), MAX, by_key=(kname, DESC), names=("counts",), work=w)
            w.check_guard()
        finally:
            w.release()
    for m, big in (((2 << 20) - 1, (2 << 20) + 5), ((1 << 20) + 1, (4 << 20) + 3)):
        assert by_key_bytes(dev, 2, 5, m) <= by_key_bytes(dev, 2, 5, big) and by_key_bytes(dev, 5, 2, m) <= by_key_bytes(dev, 5, 2, big)
    # one byte short
    m = 5000
    kin = Guarded(dev, rng.integers(0, 99, size=m).astype(np.uint32), seed=1)
    vin = Guarded(dev, rng.integers(0, 99, size=m).astype(np.uint32), seed=2)
    out = Outputs(dev, np.uint32, np.uint32, m)
    w = Guarded(dev, nbytes=by_key_bytes(dev, 0, 0, m), seed=4)
    try:
        wb = by_key_bytes(dev, 0, 0, m)
        rc = lib.adlhip_reduce_by_key_typed(dev._h, 0, ASC, kin.ptr(), 0, SUM, vin.ptr(), m, out.ptr("unique"), out.ptr("reduced"),
                                            out.ptr("counts"), out.ptr("offsets"), out.ptr("count"), w.ptr(), wb - 1)
        assert rc == 1 and str(wb) in lib_err(), lib_err()
        wb = runs_bytes(dev, 4, 0, m)
        rc = lib.adlhip_reduce_runs(dev._h, 4, kin.ptr(), 0, SUM, vin.ptr(), m, out.ptr("unique"), out.ptr("reduced"), out.ptr("counts"),
                                    out.ptr("offsets"), out.ptr("count"), w.ptr(), wb - 1)
        assert rc == 1 and str(wb) in lib_err(), lib_err()
        out.untouched()
    finally:
        for b in (kin, vin, w):
            b.release()
        out.release()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32, I32 = 2, 1
    n = 5000
    rng = np.random.default_rng(71)
    kbits = rng.integers(0, 99, size=n).astype(np.uint32)
    vbits = rng.integers(0, 99, size=n).astype(np.uint32)
    kin = Guarded(dev, kbits, seed=1)
    vin = Guarded(dev, vbits, seed=2)
    out = Outputs(dev, np.uint32, np.uint32, n)
    wb = by_key_bytes(dev, F32, I32, n)
    w = Guarded(dev, nbytes=wb, seed=4)
    sz = ctypes.c_size_t()

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    def pick(v, name):
        return out.ptr(name) if v == 0 else v

    def by_key(key_type=F32, order=ASC, keys=0, value_type=I32, op=SUM, vals=0, m=n, u=0, r=0, c=0, o=0, cnt=0, work=0, work_bytes=wb):
        """0 = the proper buffer; anything else replaces it"""
        return lib.adlhip_reduce_by_key_typed(dev._h, key_type, order, kin.ptr() if keys == 0 else keys, value_type, op,
                                              vin.ptr() if vals == 0 else vals, m, pick(u, "unique"), pick(r, "reduced"), pick(c, "counts"),
                                              pick(o, "offsets"), pick(cnt, "count"), w.ptr() if work == 0 else work, work_bytes)

    def runs(key_bytes=4, keys=0, value_type=I32, op=SUM, vals=0, m=n, u=0, r=0, c=0, o=0, cnt=0, work=0, work_bytes=wb):
        return lib.adlhip_reduce_runs(dev._h, key_bytes, kin.ptr() if keys == 0 else keys, value_type, op, vin.ptr() if vals == 0 else vals, m,
                                      pick(u, "unique"), pick(r, "reduced"), pick(c, "counts"), pick(o, "offsets"), pick(cnt, "count"),
                                      w.ptr() if work == 0 else work, work_bytes)

    def off(name, nbytes):
        return ctypes.c_void_p(out.bufs[name].buf.m_ptr + nbytes)

    try:
        for fn, label in ((by_key, "reduce by key"), (runs, "reduce runs")):
            refused(fn(keys=ctypes.c_void_p(0)), label + ": NULL keys")
            refused(fn(vals=ctypes.c_void_p(0)), label + ": NULL values")
            refused(fn(u=None), label + ": NULL d_unique_out")
            refused(fn(r=None), label + ": NULL d_reduced_out")
            refused(fn(cnt=None), label + ": NULL count word")
            refused(fn(work=ctypes.c_void_p(0)), label + ": NULL work")
            refused(fn(keys=kin.ptr(4), m=n - 1), label + ": misaligned keys")
            refused(fn(vals=vin.ptr(8), m=n - 2), label + ": misaligned values")
            refused(fn(u=off("unique", 4), m=n - 1), label + ": misaligned d_unique_out")
            refused(fn(r=off("reduced", 4), m=n - 1), label + ": misaligned d_reduced_out")
            refused(fn(c=off("counts", 4), m=n - 1), label + ": misaligned counts")
            refused(fn(o=off("offsets", 8), m=n - 2), label + ": misaligned offsets")
            refused(fn(cnt=off("count", 2)), label + ": misaligned count word")
            refused(fn(work=w.ptr(4), work_bytes=wb - 4), label + ": misaligned work")
            for inp, which in ((kin, "keys"), (vin, "values")):
                refused(fn(u=inp.ptr(16)), label + ": d_unique_out overlaps the " + which)
                refused(fn(r=inp.ptr(32)), label + ": d_reduced_out overlaps the " + which)
                refused(fn(c=inp.ptr(n * 4 - 16)), label + ": counts overlap the " + which)
                refused(fn(o=inp.ptr(0)), label + ": offsets overlap the " + which)
                refused(fn(cnt=inp.ptr(64)), label + ": the count word overlaps the " + which)
            refused(fn(m=1 << 32), label + ": n = 2^32")
            for bad in (-1, 6, 99):
                refused(fn(value_type=bad), label + ": value_type %d" % bad)
            for bad in (-1, 3):
                refused(fn(op=bad), label + ": op %d" % bad)
            assert str(wb if fn is by_key else runs_bytes(dev, 4, I32, n)) in refused(
                fn(work_bytes=(wb if fn is by_key else runs_bytes(dev, 4, I32, n)) - 1), label + ": work one byte short")
        for bad in (-1, 6, 99):
            refused(by_key(key_type=bad), "key_type %d" % bad)
            refused(lib.adlhip_reduce_by_key_scratch_bytes(dev._h, bad, I32, n, ctypes.byref(sz)), "scratch, key_type %d" % bad)
            refused(lib.adlhip_reduce_by_key_scratch_bytes(dev._h, F32, bad, n, ctypes.byref(sz)), "scratch, value_type %d" % bad)
            refused(lib.adlhip_reduce_runs_scratch_bytes(dev._h, 4, bad, n, ctypes.byref(sz)), "scratch, value_type %d" % bad)
        for bad in (-1, 2):
            refused(by_key(order=bad), "order %d" % bad)
        for bad in (0, 2, 16, -4):
            refused(runs(key_bytes=bad), "key_bytes %d" % bad)
            refused(lib.adlhip_reduce_runs_scratch_bytes(dev._h, bad, I32, n, ctypes.byref(sz)), "scratch, key_bytes %d" % bad)
        out.untouched()
        assert np.array_equal(kin.read(np.uint32), kbits) and np.array_equal(vin.read(np.uint32), vbits)
        w.check_guard()
        assert dev.getParam("debug.idle_dirty") == 0
        # n == 0 succeeds: one clear of the count word, nothing else is looked at or written
        assert by_key(m=0) == 0, lib_err()
        assert out.bufs["count"].read(np.uint32)[0] == 0
        out.bufs["count"].buf.write(out.sent["count"].view(np.uint8))
        out.untouched()
        refused(by_key(m=0, cnt=None), "n == 0 without a count word")
    finally:
        for b in (kin, vin, w):
            b.release()
        out.release()


# ---------------------------------------------------------------------------------------------
# call sequences
# ---------------------------------------------------------------------------------------------
def test_call_sequences(dev):
    """reduce calls mixed with a sort, unique and top-k on one handle; the handle's device state is idle after each step"""
    n = 90_001
    rng = np.random.default_rng(43)
    kbits = rng.integers(0, 1 << 12, size=n).astype(np.uint64)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    p = Pprims()
    sort_buf = Buffer(dev, n, np.uint32)
    fkeys = Buffer(dev, n, np.float32)
    try:
        run_reduce(dev, kbits, "f32", values_for("f32", SUM, n, rng), SUM, by_key=("i64", DESC))
        assert dev.getParam("debug.idle_dirty") == 0
        sort_buf.write(keys)
        p.radixSort(dev, sort_buf, n)
        assert np.array_equal(sort_buf.toHost(), np.sort(keys))
        assert dev.getParam("debug.idle_dirty") == 0
        run_reduce(dev, np.sort(kbits), "i64", values_for("i64", MAX, n, rng), MAX)
        assert dev.getParam("debug.idle_dirty") == 0
        fkeys.write(keys.view(np.float32))
        res = p.unique(dev, fkeys, n, counts=True)
        assert int(res.count.toHost()[0]) == np.unique(keys).size
        for b in (res.unique, res.counts, res.count):
            b.release()
        assert dev.getParam("debug.idle_dirty") == 0
        run_reduce(dev, keys, "f64", values_for("f64", SUM, n, rng), SUM, by_key=("f32", ASC), names=("counts",))
        assert dev.getParam("debug.idle_dirty") == 0
        idx = p.topk(dev, sort_buf, n, 100)
        assert np.array_equal(idx.toHost(), np.arange(100, dtype=np.uint32))       # sort_buf is sorted
        idx.release()
        assert dev.getParam("debug.idle_dirty") == 0
        run_reduce(dev, kbits.astype(np.uint32), "u32", values_for("u32", MIN, n, rng), MIN, by_key=("u32", ASC))
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        sort_buf.release()
        fkeys.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# Python mirror and torch front end (the demo's device path: tests/test_reduce_api.py)
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    n = 60_007
    rng = np.random.default_rng(81)
    kbits = rng.integers(0, 777, size=n).astype(np.uint64) * np.uint64(0x0010000000000001)
    vals = rng.integers(-8, 9, size=n).astype(np.float32)
    p = Pprims()
    keys = Buffer(dev, n, np.float64)
    values = Buffer(dev, n, np.float32)
    mine = Buffer(dev, n, np.uint32)
    try:
        keys.write(kbits.view(np.float64))
        values.write(vals)
        for op in ("sum", "min", "max"):
            exp = by_key_oracle(kbits, "f64", DESC, vals.view(np.uint32), "f32", REDUCE_OP[op])
            r_exp = exp["unique"].size
            res = p.reduceByKey(dev, keys, values, n, op=op, descending=True, counts=mine, offsets=True)
            assert int(res.count.toHost()[0]) == r_exp and res.counts is mine
            assert np.array_equal(res.unique.toHost()[:r_exp].view(np.uint64), exp["unique"])
            assert np.array_equal(res.reduced.toHost()[:r_exp].view(np.uint32), exp["reduced"])
            assert np.array_equal(mine.toHost()[:r_exp], exp["counts"]) and np.array_equal(res.offsets.toHost()[:r_exp + 1], exp["offsets"])
            for b in (res.unique, res.reduced, res.offsets, res.count):
                b.release()
        assert np.array_equal(keys.toHost().view(np.uint64), kbits) and np.array_equal(values.toHost(), vals)
        # grouped keys
        keys.write(np.sort(kbits).view(np.float64))
        exp = runs_oracle(np.sort(kbits), vals.view(np.uint32), "f32", SUM)
        res = p.reduceRuns(dev, keys, values, n)
        r_exp = exp["unique"].size
        assert res.counts is None and res.offsets is None and int(res.count.toHost()[0]) == r_exp
        assert np.array_equal(res.reduced.toHost()[:r_exp].view(np.uint32), exp["reduced"])
        for b in (res.unique, res.reduced, res.count):
            b.release()
        res = p.reduceByKey(dev, keys, values, 0, counts=True)
        assert int(res.count.toHost()[0]) == 0
        for b in (res.unique, res.reduced, res.counts, res.count):
            b.release()
        with pytest.raises(Exception):
            p.reduceByKey(dev, keys, values, n, op="mean")
    finally:
        for b in (keys, values, mine):
            b.release()
        p.close()


REDUCE_OP = {"sum": SUM, "min": MIN, "max": MAX}


@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(torch, dtype, n, seed, span=300):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-span, span, (n,), dtype=torch.int64, device="cuda", generator=g)
    if dtype.is_floating_point:
        t = torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25   # exact values; no -0 (and no +0 either), no NaN
    return t.to(dtype)


@pytest.mark.parametrize("vdtype_name", ["int32", "int64", "float32", "float64"])
@pytest.mark.parametrize("kdtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_reduce_by_key_matches_torch(sorter, kdtype_name, vdtype_name):
    import torch
    kd, vd = getattr(torch, kdtype_name), getattr(torch, vdtype_name)
    n = 50_003
    keys = _torch_input(torch, kd, n, 11)
    vals = _torch_input(torch, vd, n, 12, span=40)       # sums of quarters below 2^24: exact in every order
    keep_k, keep_v = keys.clone(), vals.clone()
    for k, v in ((keys, vals), (keys[::2], vals[::2]), (keys[1:], vals[1:])):
        uniq, inv = torch.unique(k, return_inverse=True)
        r = uniq.numel()
        want = {"sum": torch.zeros(r, dtype=vd, device="cuda").index_add_(0, inv, v),
                "min": torch.zeros(r, dtype=vd, device="cuda").scatter_reduce_(0, inv, v, "amin", include_self=False),
                "max": torch.zeros(r, dtype=vd, device="cuda").scatter_reduce_(0, inv, v, "amax", include_self=False)}
        counts = torch.bincount(inv, minlength=r)
        for op in ("sum", "min", "max"):
            u, red, c = sorter.reduce_by_key(k, v, op=op, return_counts=True)
            assert u.dtype == kd and red.dtype == vd and c.dtype == torch.int64
            assert torch.equal(u, uniq) and torch.equal(red, want[op]) and torch.equal(c, counts), op
            u, red = sorter.reduce_by_key(k, v, op=op, descending=True)
            assert torch.equal(u, uniq.flip(0)) and torch.equal(red, want[op].flip(0)), op
        # grouped keys: the sorted ones
        ks, order = torch.sort(k, stable=True)
        u, red, c = sorter.reduce_consecutive(ks, v[order], op="sum", return_counts=True)
        assert torch.equal(u, uniq) and torch.equal(red, want["sum"]) and torch.equal(c, counts)
    assert torch.equal(keys, keep_k) and torch.equal(vals, keep_v), "an input was changed"
    u, red, c = sorter.reduce_by_key(torch.empty(0, dtype=kd, device="cuda"), torch.empty(0, dtype=vd, device="cuda"), return_counts=True)
    assert u.numel() == 0 and u.dtype == kd and red.numel() == 0 and red.dtype == vd and c.dtype == torch.int64


def test_torch_sorter_reduce_is_bound_to_its_stream(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    k = torch.tensor([3, 1, 3, 2, 1, 3], dtype=torch.int32, device="cuda")
    v = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0], dtype=torch.float64, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "reduceByKey", boom)
        monkeypatch.setattr(sorter.pprims, "reduceRuns", boom)
        with pytest.raises(RuntimeError):
            sorter.reduce_by_key(k, v)
        with pytest.raises(RuntimeError):
            sorter.reduce_consecutive(k, v)
        monkeypatch.undo()
    u, red, c = sorter.reduce_by_key(k, v, return_counts=True)
    assert u.tolist() == [1, 2, 3] and red.tolist() == [18.0, 8.0, 37.0] and c.tolist() == [2, 1, 3]
    u, red = sorter.reduce_by_key(k, v, op="max", descending=True)
    assert u.tolist() == [3, 2, 1] and red.tolist() == [32.0, 8.0, 16.0]
    u, red, c = sorter.reduce_consecutive(k, v, op="min", return_counts=True)
    assert u.tolist() == [3, 1, 3, 2, 1, 3] and red.tolist() == v.tolist() and c.tolist() == [1] * 6
    for bad in (torch.zeros(6, dtype=torch.float16, device="cuda"), torch.zeros(6, dtype=torch.float32), [3.0, 1.0],
                torch.zeros((2, 3), dtype=torch.int32, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")):
        with pytest.raises((TypeError, ValueError)):
            sorter.reduce_by_key(bad, v)
        with pytest.raises((TypeError, ValueError)):
            sorter.reduce_consecutive(k, bad)
    with pytest.raises(ValueError):
        sorter.reduce_by_key(k, v, op="mean")
