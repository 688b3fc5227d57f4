"""Typed keys, order and argsort on the GPU (include/adlhip.h "typed keys, order, argsort"; oclradixsort_amd/torch_sort.py).

Expected results come from numpy (tests/typed_shapes.py) and are stated independently of the key codec's formula: a key's ordinal is its bit pattern
read as sign-magnitude (s = the bits as a signed integer; ordinal = s if s >= 0 else -(s & MAX) - 1) for floats, the value itself
for integers, and the expected permutation is the stable argsort of the ordinal (descending: of the negated ordinal, which is
exact in int64 for 4-byte keys and taken on (high, low) halves for 8-byte keys).  Everything is compared bit for bit.

Every buffer a call may touch carries 64 sentinel elements behind its n elements, checked after every call.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded: a torch wheel that bundles its HIP runtime must load it first,
#                            the back-end then shares it; the other way round the process holds two runtimes and torch sees no GPU)

from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from typed_shapes import ASC, DESC, SPECIALS, TYPES, expected_perm, ordinal_halves   # the expected order, from numpy

pytestmark = pytest.mark.gpu

TYPE_IDS = [t[0] for t in TYPES]
ORDER_IDS = ["asc", "desc"]
SENTINELS = 64


def random_bits(udt, n, seed, few=False):
    """n random bit patterns with the specials spliced in; few: drawn from 37 values (+ the specials), so that ties abound."""
    rng = np.random.default_rng(seed)
    w = np.dtype(udt).itemsize
    if few:
        pool = np.frombuffer(rng.bytes(w * 37), dtype=udt)
        x = pool[rng.integers(0, 37, size=n)]
    elif w == 4:
        x = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    else:
        x = np.frombuffer(rng.bytes(8 * n), dtype=np.uint64).copy()
    sp = SPECIALS[w]
    if n >= 8:
        at = rng.choice(n, size=min(n // 2, 3 * sp.size), replace=False)
        x[at] = np.resize(sp, at.size)
    return np.ascontiguousarray(x, dtype=udt)


# ---------------------------------------------------------------------------------------------
# device plumbing: raw byte buffers with sentinels behind the payload
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    DeviceUtils.deallocate(d)


def lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


class Guarded:
    """`payload` (any numpy array, taken as bytes) -- or nbytes of scratch, contents arbitrary -- on the device, followed by a guard of
    known bytes."""

    def __init__(self, dev, payload=None, nbytes=None, guard_bytes=256, seed=1):
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
            self.buf.write(self.guard, dstOffsetNElems=self.nbytes)

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.buf.m_ptr + offset)

    def check_guard(self):
        got = np.empty(self.guard.size, np.uint8)
        self.buf.read(got, srcOffsetNElems=self.nbytes)
        DeviceUtils.waitForCompletion(self.dev)
        assert np.array_equal(got, self.guard), "bytes behind the buffer were written"

    def read(self, dtype):
        """payload as dtype; asserts the guard is intact"""
        raw = self.buf.toHost()
        assert np.array_equal(raw[self.nbytes:], self.guard), "bytes behind the buffer were written"
        return raw[:self.nbytes].view(dtype)

    def release(self):
        self.buf.release()


def scratch_sizes(dev, kt, mode, vb, n):
    tk, tv, wb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = _lib.load().adlhip_sort_typed_scratch_bytes(dev._h, kt, mode, vb, n, ctypes.byref(tk), ctypes.byref(tv), ctypes.byref(wb))
    assert rc == 0, lib_err()
    return tk.value, tv.value, wb.value


def align16(nbytes):
    """the partner arrays hold n elements; a buffer's size is rounded to the 16 bytes of its alignment only, so that the sentinels sit
    right behind element n"""
    return max((nbytes + 15) // 16 * 16, 16)


def guard_of(dtype):
    return SENTINELS * np.dtype(dtype).itemsize


def sort_keys(dev, kt, order, bits):
    """adlhip_sort_keys_typed on the bit patterns; returns the sorted bit patterns"""
    n = bits.size
    tk, _, wb = scratch_sizes(dev, kt, 0, 0, n)
    k = Guarded(dev, bits, guard_bytes=guard_of(bits.dtype), seed=2)
    assert tk >= bits.nbytes
    t = Guarded(dev, nbytes=align16(bits.nbytes), guard_bytes=guard_of(bits.dtype), seed=3)
    w = Guarded(dev, nbytes=max(wb, 16), seed=4)
    try:
        rc = _lib.load().adlhip_sort_keys_typed(dev._h, kt, order, k.ptr(), t.ptr(), w.ptr(), wb, n)
        assert rc == 0, lib_err()
        t.check_guard()
        w.check_guard()
        return k.read(bits.dtype)
    finally:
        for b in (k, t, w):
            b.release()


def argsort(dev, kt, order, bits, with_keys_out):
    """adlhip_argsort_typed; returns (index, sorted bit patterns or None); asserts the input is intact"""
    n = bits.size
    _, _, wb = scratch_sizes(dev, kt, 2, 0, n)
    k = Guarded(dev, bits, guard_bytes=guard_of(bits.dtype), seed=5)
    ko = Guarded(dev, nbytes=bits.nbytes or 16, guard_bytes=guard_of(bits.dtype), seed=6) if with_keys_out else None
    io = Guarded(dev, nbytes=4 * n or 16, guard_bytes=guard_of(np.uint32), seed=7)
    w = Guarded(dev, nbytes=max(wb, 16), seed=8)
    try:
        rc = _lib.load().adlhip_argsort_typed(dev._h, kt, order, k.ptr(), ko.ptr() if ko else None, io.ptr(), w.ptr(), wb, n)
        assert rc == 0, lib_err()
        w.check_guard()
        assert np.array_equal(k.read(bits.dtype), bits), "argsort changed d_keys_in"
        return io.read(np.uint32)[:n], (ko.read(bits.dtype)[:n] if ko else None)
    finally:
        for b in (k, ko, io, w):
            if b is not None:
                b.release()


def sort_pairs(dev, kt, order, bits, vals):
    """adlhip_sort_pairs_typed; vals: (n,) uint32 / uint64 or (n, 4) uint32 (16-byte values); returns (keys, values)"""
    n = bits.size
    vb = vals.nbytes // max(n, 1) if n else vals.dtype.itemsize * (4 if vals.ndim == 2 else 1)
    tk, tv, wb = scratch_sizes(dev, kt, 1, vb, n)
    k = Guarded(dev, bits, guard_bytes=guard_of(bits.dtype), seed=9)
    v = Guarded(dev, vals, guard_bytes=SENTINELS * vb, seed=10)
    assert tv >= vals.nbytes and (tk == 0 or tk >= bits.nbytes)
    tkb = Guarded(dev, nbytes=align16(bits.nbytes), guard_bytes=guard_of(bits.dtype), seed=11)
    tvb = Guarded(dev, nbytes=align16(vals.nbytes), guard_bytes=SENTINELS * vb, seed=12)
    w = Guarded(dev, nbytes=max(wb, 16), seed=13)
    try:
        rc = _lib.load().adlhip_sort_pairs_typed(dev._h, kt, order, k.ptr(), v.ptr(), vb, tkb.ptr() if tk else None, tvb.ptr(), w.ptr(), wb, n)
        assert rc == 0, lib_err()
        for b in (tkb, tvb, w):
            b.check_guard()
        return k.read(bits.dtype), v.read(vals.dtype).reshape(vals.shape)
    finally:
        for b in (k, v, tkb, tvb, w):
            b.release()


def values_for(n, vb):
    """i-derived patterns of vb bytes"""
    i = np.arange(n, dtype=np.uint64)
    if vb == 4:
        return (i * np.uint64(2654435761) + np.uint64(12345)).astype(np.uint32)
    if vb == 8:
        return i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
    i32 = i.astype(np.uint32)
    return np.ascontiguousarray(np.stack([i32, ~i32, i32 * np.uint32(3), i32 ^ np.uint32(0x5a5a5a5a)], axis=1))


# ---------------------------------------------------------------------------------------------
# codec
# ---------------------------------------------------------------------------------------------
CODEC_SIZES = [0, 1, 3, 4, 5, 255, 256, 257, (5 << 20) + 3]   # the last exceeds one grid sweep: stride loop + vector tail
# the body takes four vectors per thread and turn while that many are left: 4096 workgroups x 256 threads x 4 vectors of 16 bytes
# = 64 MiB per turn on 256 CUs.  This many bytes give two such turns, single-vector turns behind them and a scalar tail
CODEC_LONG_BYTES = (132 << 20) + 4096
_CODEC_INPUT = {}


def codec_input(udt):
    w = np.dtype(udt).itemsize
    if w not in _CODEC_INPUT:
        _CODEC_INPUT[w] = random_bits(udt, CODEC_LONG_BYTES // w + 3, 77 + w)
    return _CODEC_INPUT[w]


def run_codec(dev, fn, kt, order, src_bits, in_place):
    n = src_bits.size
    g = guard_of(src_bits.dtype)
    s = Guarded(dev, src_bits, guard_bytes=g, seed=20) if n else Guarded(dev, nbytes=16, guard_bytes=g, seed=20)
    d = s if in_place else Guarded(dev, nbytes=src_bits.nbytes or 16, guard_bytes=g, seed=21)
    try:
        rc = fn(dev._h, kt, order, d.ptr(), s.ptr(), n)
        assert rc == 0, lib_err()
        out = d.read(src_bits.dtype)[:n].copy()
        if not in_place and n:
            assert np.array_equal(s.read(src_bits.dtype), src_bits), "the codec wrote its source"
        return out
    finally:
        s.release()
        if d is not s:
            d.release()


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_codec_round_trip_and_order(dev, name, kt, dt, udt, order):
    lib = _lib.load()
    full = codec_input(udt)
    for n in CODEC_SIZES:
        x = full[:n]
        for in_place in (False, True):
            enc = run_codec(dev, lib.adlhip_key_encode, kt, order, x, in_place)
            back = run_codec(dev, lib.adlhip_key_decode, kt, order, enc, in_place)
            assert np.array_equal(back, x), (name, n, in_place)
            if n >= 2:   # unsigned order of the encoded keys == order of the ordinals, pair by neighbouring pair
                hi, lo = ordinal_halves(x, name)
                less = (hi[:-1] < hi[1:]) | ((hi[:-1] == hi[1:]) & (lo[:-1] < lo[1:]))
                same = (hi[:-1] == hi[1:]) & (lo[:-1] == lo[1:])
                if order == DESC:
                    assert np.array_equal(enc[:-1] > enc[1:], less), (name, n)
                else:
                    assert np.array_equal(enc[:-1] < enc[1:], less), (name, n)
                assert np.array_equal(enc[:-1] == enc[1:], same), (name, n)
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_codec_round_trip_over_several_turns_of_the_unrolled_body(dev, name, kt, dt, udt, order):
    lib = _lib.load()
    x = codec_input(udt)
    enc = run_codec(dev, lib.adlhip_key_encode, kt, order, x, True)
    for part in (slice(0, 1 << 20), slice(x.size - (1 << 20), x.size)):   # order, on both ends
        hi, lo = ordinal_halves(x[part], name)
        less = (hi[:-1] < hi[1:]) | ((hi[:-1] == hi[1:]) & (lo[:-1] < lo[1:]))
        e = enc[part]
        assert np.array_equal(e[:-1] > e[1:] if order == DESC else e[:-1] < e[1:], less)
    assert np.array_equal(run_codec(dev, lib.adlhip_key_decode, kt, order, enc, True), x)


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_codec_is_strictly_monotone_on_the_specials(dev, name, kt, dt, udt, order):
    sp = np.unique(SPECIALS[np.dtype(udt).itemsize])
    hi, lo = ordinal_halves(sp, name)
    by_ordinal = sp[np.lexsort((lo, hi))]
    if name[0] == "f":   # the hand-made vector, in the order IEEE-754 totalOrder gives it: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
        as_float = by_ordinal.view(dt)
        fin = np.isfinite(as_float)
        first_finite, last_finite = np.flatnonzero(fin)[0], np.flatnonzero(fin)[-1]
        assert np.isnan(as_float[:first_finite - 1]).all() and np.isneginf(as_float[first_finite - 1])
        assert np.isposinf(as_float[last_finite + 1]) and np.isnan(as_float[last_finite + 2:]).all()
        assert np.all(np.diff(as_float[first_finite:last_finite + 1].astype(np.float64)) >= 0)
        z = np.flatnonzero(as_float == 0)
        assert z.size == 2 and np.signbit(as_float[z[0]]) and not np.signbit(as_float[z[1]])
    enc = run_codec(dev, _lib.load().adlhip_key_encode, kt, order, by_ordinal, False)
    step = np.diff(enc.astype(object))
    assert all(s < 0 for s in step) if order == DESC else all(s > 0 for s in step), (name, [hex(int(e)) for e in enc])


# ---------------------------------------------------------------------------------------------
# keys only
# ---------------------------------------------------------------------------------------------
KEY_SIZES = {4: [1000, 300_000, (3 << 20) + 17], 8: [1000, 300_000]}   # one n per size class of the unsigned sort underneath


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_keys_only(dev, name, kt, dt, udt, order):
    for n in KEY_SIZES[np.dtype(udt).itemsize]:
        x = random_bits(udt, n, 1000 + kt)
        got = sort_keys(dev, kt, order, x)
        assert np.array_equal(got, x[expected_perm(x, name, order)]), (name, n)
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", [t for t in TYPES if t[0][0] == "f"], ids=["f32", "f64"])
def test_keys_only_standard_normal(dev, name, kt, dt, udt, order):
    n = KEY_SIZES[np.dtype(udt).itemsize][-1]
    x = np.random.default_rng(5).standard_normal(n).astype(dt).view(udt)
    before = dev.getParam("stat.net_runs")
    got = sort_keys(dev, kt, order, x)
    print("%s n=%d standard normal: stat.net_runs %d -> %d" % (name, n, before, dev.getParam("stat.net_runs")))
    assert np.array_equal(got, x[expected_perm(x, name, order)])
    want = np.sort(x.view(dt))   # no NaN, no -0 here (almost surely): numpy's own float order agrees
    assert np.array_equal(got.view(dt), want[::-1] if order == DESC else want)


# ---------------------------------------------------------------------------------------------
# argsort and pairs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_argsort_and_pairs_are_stable(dev, name, kt, dt, udt, order):
    for n in KEY_SIZES[np.dtype(udt).itemsize]:
        x = random_bits(udt, n, 2000 + kt, few=True)
        perm = expected_perm(x, name, order)
        # ties keep input order, descending too: inside a run of equal keys the expected indices ascend
        tie = x[perm][:-1] == x[perm][1:]
        assert tie.sum() > n // 2 and np.all(perm[1:][tie] > perm[:-1][tie])
        idx, none = argsort(dev, kt, order, x, False)
        assert none is None and np.array_equal(idx, perm.astype(np.uint32)), (name, n)
        idx, ks = argsort(dev, kt, order, x, True)
        assert np.array_equal(idx, perm.astype(np.uint32)) and np.array_equal(ks, x[perm]), (name, n)
        for vb in (4, 8, 16):
            v = values_for(n, vb)
            gk, gv = sort_pairs(dev, kt, order, x, v)
            assert np.array_equal(gk, x[perm]), (name, n, vb)
            assert np.array_equal(gv, v[perm]), (name, n, vb)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# identity, bounds, idle state, refusals
# ---------------------------------------------------------------------------------------------
def test_u32_ascending_launches_no_codec_kernel(dev):
    x = random_bits(np.uint32, 300_000, 31)
    dev.toggleProfiling(True)
    try:
        dev.profile(reset=True)
        assert np.array_equal(sort_keys(dev, 0, ASC, x), np.sort(x))
        names = set(dev.profile(reset=True))
        assert names and not any("encode" in k or "decode" in k or "typed" in k for k in names), names
        y = random_bits(np.uint64, 1000, 32)
        assert np.array_equal(sort_keys(dev, 3, ASC, y), np.sort(y))
        names = set(dev.profile(reset=True))
        assert names and not any("encode" in k or "decode" in k or "typed" in k for k in names), names
        # positive control: a signed sort does show them
        sort_keys(dev, 1, ASC, x)
        names = set(dev.profile(reset=True))
        assert "key_encode" in names and "key_decode" in names, names
    finally:
        dev.toggleProfiling(False)


@pytest.mark.parametrize("n", [257, 300_001])
def test_every_call_stays_in_bounds_and_leaves_the_handle_idle(dev, n):
    """(sort_keys / argsort / sort_pairs / run_codec check the sentinels behind every buffer they pass)"""
    lib = _lib.load()
    for name, kt, dt, udt in TYPES:
        x = random_bits(udt, n, 3000 + kt, few=True)
        for order in (ASC, DESC):
            perm = expected_perm(x, name, order)
            enc = run_codec(dev, lib.adlhip_key_encode, kt, order, x, True)
            assert dev.getParam("debug.idle_dirty") == 0
            assert np.array_equal(run_codec(dev, lib.adlhip_key_decode, kt, order, enc, False), x)
            assert dev.getParam("debug.idle_dirty") == 0
            assert np.array_equal(sort_keys(dev, kt, order, x), x[perm])
            assert dev.getParam("debug.idle_dirty") == 0
            idx, ks = argsort(dev, kt, order, x, True)
            assert np.array_equal(idx, perm.astype(np.uint32)) and np.array_equal(ks, x[perm])
            assert dev.getParam("debug.idle_dirty") == 0
            vb = (4, 8, 16)[(kt + order) % 3]
            v = values_for(n, vb)
            gk, gv = sort_pairs(dev, kt, order, x, v)
            assert np.array_equal(gk, x[perm]) and np.array_equal(gv, v[perm])
            assert dev.getParam("debug.idle_dirty") == 0


def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    n = 5000
    x = random_bits(np.uint32, n, 41)
    v = values_for(n, 4)
    tk0, _, wb0 = scratch_sizes(dev, 2, 0, 0, n)
    _, tv1, wb1 = scratch_sizes(dev, 2, 1, 4, n)
    _, _, wb2 = scratch_sizes(dev, 2, 2, 0, n)
    pad = 64
    k = Guarded(dev, np.concatenate([x, x[:pad]]), seed=50)      # (room for the + 4 byte pointers)
    vv = Guarded(dev, np.concatenate([v, v[:pad]]), seed=51)
    t = Guarded(dev, nbytes=max(tk0, tv1) + 256, seed=52)
    t2 = Guarded(dev, nbytes=max(tk0, tv1) + 256, seed=53)
    out = Guarded(dev, nbytes=4 * n + 256, seed=54)
    w = Guarded(dev, nbytes=max(wb0, wb1, wb2) + 256, seed=55)
    bufs = (k, vv, t, t2, out, w)
    before = [b.read(np.uint8).copy() for b in bufs]
    dev.toggleProfiling(True)
    dev.profile(reset=True)

    def refused(rc, what):
        assert rc != 0, what + " was accepted"
        assert lib_err(), what + ": no message"
        return lib_err()

    try:
        F32 = 2
        # misaligned pointers (base + 4 bytes), one argument at a time
        refused(lib.adlhip_key_encode(dev._h, F32, ASC, k.ptr(4), k.ptr(), n), "encode to a misaligned dst")
        refused(lib.adlhip_key_decode(dev._h, F32, ASC, k.ptr(), k.ptr(4), n), "decode from a misaligned src")
        refused(lib.adlhip_sort_keys_typed(dev._h, F32, ASC, k.ptr(4), t.ptr(), w.ptr(), wb0, n), "sort_keys, misaligned keys")
        refused(lib.adlhip_sort_keys_typed(dev._h, F32, ASC, k.ptr(), t.ptr(4), w.ptr(), wb0, n), "sort_keys, misaligned tmp")
        refused(lib.adlhip_sort_keys_typed(dev._h, F32, ASC, k.ptr(), t.ptr(), w.ptr(4), wb0, n), "sort_keys, misaligned work")
        refused(lib.adlhip_sort_pairs_typed(dev._h, F32, ASC, k.ptr(), vv.ptr(4), 4, t.ptr(), t2.ptr(), w.ptr(), wb1, n), "sort_pairs, misaligned values")
        refused(lib.adlhip_sort_pairs_typed(dev._h, F32, ASC, k.ptr(), vv.ptr(), 4, t.ptr(), t2.ptr(4), w.ptr(), wb1, n), "sort_pairs, misaligned tmp values")
        refused(lib.adlhip_argsort_typed(dev._h, F32, ASC, k.ptr(4), None, out.ptr(), w.ptr(), wb2, n), "argsort, misaligned keys")
        refused(lib.adlhip_argsort_typed(dev._h, F32, ASC, k.ptr(), t.ptr(), out.ptr(4), w.ptr(), wb2, n), "argsort, misaligned index")
        # a work buffer one byte too small: the message names the size needed
        assert str(wb0) in refused(lib.adlhip_sort_keys_typed(dev._h, F32, ASC, k.ptr(), t.ptr(), w.ptr(), wb0 - 1, n), "sort_keys, small work")
        assert str(wb1) in refused(lib.adlhip_sort_pairs_typed(dev._h, F32, ASC, k.ptr(), vv.ptr(), 4, t.ptr(), t2.ptr(), w.ptr(), wb1 - 1, n), "sort_pairs, small work")
        assert str(wb2) in refused(lib.adlhip_argsort_typed(dev._h, F32, ASC, k.ptr(), None, out.ptr(), w.ptr(), wb2 - 1, n), "argsort, small work")
        for bad in (-1, 6):   # key_type
            refused(lib.adlhip_key_encode(dev._h, bad, ASC, k.ptr(), k.ptr(), n), "encode, key_type %d" % bad)
            refused(lib.adlhip_key_decode(dev._h, bad, ASC, k.ptr(), k.ptr(), n), "decode, key_type %d" % bad)
            refused(lib.adlhip_sort_keys_typed(dev._h, bad, ASC, k.ptr(), t.ptr(), w.ptr(), wb0, n), "sort_keys, key_type %d" % bad)
            refused(lib.adlhip_sort_pairs_typed(dev._h, bad, ASC, k.ptr(), vv.ptr(), 4, t.ptr(), t2.ptr(), w.ptr(), wb1, n), "sort_pairs, key_type %d" % bad)
            refused(lib.adlhip_argsort_typed(dev._h, bad, ASC, k.ptr(), None, out.ptr(), w.ptr(), wb2, n), "argsort, key_type %d" % bad)
            sz = ctypes.c_size_t()
            refused(lib.adlhip_sort_typed_scratch_bytes(dev._h, bad, 0, 0, n, ctypes.byref(sz), ctypes.byref(sz), ctypes.byref(sz)), "scratch, key_type %d" % bad)
        for bad in (-1, 2):   # order
            refused(lib.adlhip_key_encode(dev._h, F32, bad, k.ptr(), k.ptr(), n), "encode, order %d" % bad)
            refused(lib.adlhip_sort_keys_typed(dev._h, F32, bad, k.ptr(), t.ptr(), w.ptr(), wb0, n), "sort_keys, order %d" % bad)
            refused(lib.adlhip_sort_pairs_typed(dev._h, F32, bad, k.ptr(), vv.ptr(), 4, t.ptr(), t2.ptr(), w.ptr(), wb1, n), "sort_pairs, order %d" % bad)
            refused(lib.adlhip_argsort_typed(dev._h, F32, bad, k.ptr(), None, out.ptr(), w.ptr(), wb2, n), "argsort, order %d" % bad)
        for bad in (2, 0, 32):   # value_bytes
            refused(lib.adlhip_sort_pairs_typed(dev._h, F32, ASC, k.ptr(), vv.ptr(), bad, t.ptr(), t2.ptr(), w.ptr(), wb1, n), "sort_pairs, value_bytes %d" % bad)
            sz = ctypes.c_size_t()
            refused(lib.adlhip_sort_typed_scratch_bytes(dev._h, F32, 1, bad, n, ctypes.byref(sz), ctypes.byref(sz), ctypes.byref(sz)), "scratch, value_bytes %d" % bad)
        # null buffers
        refused(lib.adlhip_sort_keys_typed(dev._h, F32, ASC, None, t.ptr(), w.ptr(), wb0, n), "sort_keys, null keys")
        refused(lib.adlhip_argsort_typed(dev._h, F32, ASC, k.ptr(), None, None, w.ptr(), wb2, n), "argsort, null index")
        assert dev.profile(reset=True) == {}, "a refused call launched a kernel"
        for b, was in zip(bufs, before):
            assert np.array_equal(b.read(np.uint8), was), "a refused call wrote a buffer"
        # n == 0 succeeds and launches nothing, whatever the pointers
        assert lib.adlhip_sort_keys_typed(dev._h, F32, DESC, None, None, None, 0, 0) == 0
        assert lib.adlhip_sort_pairs_typed(dev._h, F32, DESC, None, None, 8, None, None, None, 0, 0) == 0
        assert lib.adlhip_argsort_typed(dev._h, F32, DESC, None, None, None, None, 0, 0) == 0
        assert lib.adlhip_key_encode(dev._h, F32, DESC, None, None, 0) == 0
        assert dev.profile(reset=True) == {}
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.toggleProfiling(False)
        for b in bufs:
            b.release()


# ---------------------------------------------------------------------------------------------
# the Python mirror
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    p = Pprims()
    n = 20_011
    try:
        for name, kt, dt, udt in TYPES:
            x = random_bits(udt, n, 4000 + kt, few=True)
            for descending in (False, True):
                perm = expected_perm(x, name, DESC if descending else ASC)
                kb = Buffer(dev, n, dt)
                vb = Buffer(dev, n, np.uint64)
                ko = Buffer(dev, n, dt)
                try:
                    kb.write(x.view(dt))
                    v = values_for(n, 8)
                    vb.write(v)
                    ib = p.argsort(dev, kb, n, descending=descending, keysOut=ko)
                    assert ib.dtype == np.uint32 and np.array_equal(ib.toHost(), perm.astype(np.uint32))
                    ib.release()
                    assert np.array_equal(ko.toHost().view(udt), x[perm])
                    assert np.array_equal(kb.toHost().view(udt), x)
                    p.sortPairs(dev, kb, vb, n, descending=descending)
                    assert np.array_equal(kb.toHost().view(udt), x[perm]) and np.array_equal(vb.toHost(), v[perm])
                    kb.write(x.view(dt))
                    p.sortKeys(dev, kb, n, descending=descending)
                    assert np.array_equal(kb.toHost().view(udt), x[perm])
                finally:
                    for b in (kb, vb, ko):
                        b.release()
        from oclradixsort_amd import AdlHipError
        b16 = Buffer(dev, 16, np.uint16)
        with pytest.raises(AdlHipError):
            p.sortKeys(dev, b16, 16)
        b16.release()
    finally:
        p.close()


# ---------------------------------------------------------------------------------------------
# torch front end
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(torch, dtype, n):
    g = torch.Generator(device="cuda").manual_seed(11)
    if dtype.is_floating_point:
        t = torch.randn(n, dtype=dtype, device="cuda", generator=g)
        return torch.where(t == 0, torch.ones_like(t), t)   # no -0 (and no +0 either)
    return torch.randint(-500, 500, (n,), dtype=dtype, device="cuda", generator=g)   # many ties


@pytest.mark.parametrize("descending", [False, True], ids=ORDER_IDS)
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_matches_torch_sort(sorter, dtype_name, descending):
    import torch
    dtype = getattr(torch, dtype_name)
    n = 100_003
    t = _torch_input(torch, dtype, n)
    keep = t.clone()
    values, indices = sorter.sort(t, descending=descending)
    want_v, want_i = torch.sort(t, stable=True, descending=descending)
    torch.cuda.synchronize()
    assert values.dtype == dtype and indices.dtype == torch.int64 and values.is_contiguous()
    assert torch.equal(values, want_v) and torch.equal(indices, want_i)
    assert torch.equal(sorter.argsort(t, descending=descending), want_i)
    assert torch.equal(t, keep), "the input was changed"
    # a strided view
    half = t[::2]
    assert not half.is_contiguous()
    values, indices = sorter.sort(half, descending=descending)
    want_v, want_i = torch.sort(half, stable=True, descending=descending)
    assert torch.equal(values, want_v) and torch.equal(indices, want_i)
    assert torch.equal(t, keep), "the input was changed"
    # contiguous views that start at an odd offset: the ABI wants 16-byte alignment, the front end sees to it
    for view in (t[1:], t[3:]):
        assert view.is_contiguous() and view.data_ptr() % 16
        values, indices = sorter.sort(view, descending=descending)
        want_v, want_i = torch.sort(view, stable=True, descending=descending)
        assert torch.equal(values, want_v) and torch.equal(indices, want_i)
        assert torch.equal(sorter.argsort(view, descending=descending), want_i)
    assert torch.equal(t, keep), "the input was changed"
    # empty, aligned and not
    for view in (t[:0], t[1:1]):
        values, indices = sorter.sort(view, descending=descending)
        assert values.numel() == 0 and indices.numel() == 0 and indices.dtype == torch.int64 and values.dtype == dtype
        assert sorter.argsort(view, descending=descending).numel() == 0


@pytest.mark.parametrize("descending", [False, True], ids=ORDER_IDS)
@pytest.mark.parametrize("kind", ["int64-in-1000", "float64-normal", "float64-nan30"])
def test_torch_sorter_on_value_shaped_keys_above_one_mi(sorter, kind, descending):
    """The torch front end against torch itself where each key dword sends its pair sort somewhere else (tests/typed_shapes.py): small
    int64 values (two high dwords, 2001 low ones) and float64 normals (distinct low dwords, high ones under one top byte) have no NaN
    and no -0, so values and indices are torch.sort(stable=True)'s bit for bit; with 30 % (+)NaN the finite keys are torch's and the
    NaNs are last ascending, first descending, in index order -- where totalOrder and torch both put them."""
    import torch
    n = (1 << 20) + 77
    g = torch.Generator(device="cuda").manual_seed(5)
    if kind == "int64-in-1000":
        t = torch.randint(-1000, 1001, (n,), dtype=torch.int64, device="cuda", generator=g)
    else:
        t = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
        t = torch.where(t == 0, torch.ones_like(t), t)   # no -0
        if kind == "float64-nan30":
            t[torch.rand(n, device="cuda", generator=g) < 0.30] = float("nan")
    keep = t.clone()
    values, indices = sorter.sort(t, descending=descending)
    want_v, want_i = torch.sort(t, stable=True, descending=descending)
    torch.cuda.synchronize()
    if kind != "float64-nan30":
        assert torch.equal(values, want_v) and torch.equal(indices, want_i)
    else:
        nan = torch.isnan(t)
        k = int(nan.sum())
        assert 0.29 * n < k < 0.31 * n and not torch.signbit(t[nan]).any()
        where_nan = torch.nonzero(nan).reshape(-1)
        fin = slice(k, n) if descending else slice(0, n - k)
        nans = slice(0, k) if descending else slice(n - k, n)
        assert torch.equal(values[fin], want_v[fin]) and torch.equal(indices[fin], want_i[fin])
        assert torch.isnan(values[nans]).all() and torch.equal(indices[nans], where_nan)
        assert torch.isnan(want_v[nans]).all()
    assert torch.equal(t.view(torch.int64), keep.view(torch.int64)), "the input was changed"   # (bits: a NaN equals no NaN)


def test_torch_sorter_refuses_before_any_native_call(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    monkeypatch.setattr(sorter.pprims, "argsort", boom)
    monkeypatch.setattr(sorter.device, "checkFault", boom)
    for bad in (torch.zeros(8, dtype=torch.float16, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda"),
                torch.zeros((4, 4), dtype=torch.float32, device="cuda"), torch.zeros(8, dtype=torch.float32), [3.0, 1.0]):
        with pytest.raises((TypeError, ValueError)):
            sorter.sort(bad)
        with pytest.raises((TypeError, ValueError)):
            sorter.argsort(bad, descending=True)


def test_torch_sorter_is_bound_to_the_stream_it_was_made_on(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.arange(100, 0, -1, dtype=torch.int32, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "argsort", boom)
        with pytest.raises(RuntimeError):
            sorter.sort(t)
        monkeypatch.undo()
    values, indices = sorter.sort(t)   # back on the sorter's stream
    assert torch.equal(values, torch.arange(1, 101, dtype=torch.int32, device="cuda"))
    assert torch.equal(indices, torch.arange(99, -1, -1, dtype=torch.int64, device="cuda"))
