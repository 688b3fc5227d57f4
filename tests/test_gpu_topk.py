"""Top-k on the GPU (include/adlhip.h "top-k"; oclradixsort_amd/csrc/select_kernels.hpp; TorchSorter.topk).

The expected output is stated independently of the key codec, as in test_gpu_typed_sort.py: a key's ordinal is its bit pattern read
as sign-magnitude for floats, the value itself for integers; the expected permutation is the stable argsort of the ordinal
(descending: of the negated ordinal) and top-k is its first k entries with the keys at those positions.  Everything is compared bit
for bit, nothing is excluded, there is no tolerance.

Every device buffer carries sentinels behind its payload, checked after each call: the input, both outputs (sized exactly k) and the
work buffer (sized exactly the reported bytes).  The input is compared with its original afterwards.

T below is the tile of the selection kernels: 256 threads x 4 vectors of 16 bytes = 4096 4-byte keys / 2048 8-byte keys.  The
implementation has no single-workgroup finish; the "hand-off limit" of the survivor cases is one tile (4096 4-byte keys), the size at
which a survivor list stops fitting one workgroup's single trip.
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
ALGOS = (1, 0)   # "topk.algo": the selection, the full argsort
TILE = {4: 4096, 8: 2048}

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
# the expected order, from numpy (the helper lines of test_gpu_typed_sort.py)
# ---------------------------------------------------------------------------------------------
def ordinal_halves(bits, name):
    w = bits.dtype.itemsize
    if name[0] == "u":
        if w == 4:
            return bits.astype(np.int64), np.zeros(bits.size, np.int64)
        return (bits >> np.uint64(32)).astype(np.int64), (bits & np.uint64(0xffffffff)).astype(np.int64)
    s = bits.view(np.int32 if w == 4 else np.int64).astype(np.int64)
    if name[0] == "f":   # sign-magnitude
        mx = np.int64(0x7fffffff if w == 4 else 0x7fffffffffffffff)
        s = np.where(s >= 0, s, -(s & mx) - 1)
    if w == 4:
        return s, np.zeros(bits.size, np.int64)
    return s >> np.int64(32), s & np.int64(0xffffffff)


def expected_perm(bits, name, order):
    hi, lo = ordinal_halves(bits, name)
    if order == DESC:
        hi, lo = -hi, -lo
    if bits.dtype.itemsize == 4:
        return np.argsort(hi, kind="stable")
    return np.lexsort((lo, hi))   # stable; the last key is the primary one


def random_bits(udt, n, seed, few=False):
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
    if n >= 8 and not few:
        at = rng.choice(n, size=min(n // 2, 3 * sp.size), replace=False)
        x[at] = np.resize(sp, at.size)
    return np.ascontiguousarray(x, dtype=udt)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("topk.algo", -1)
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


def topk_bytes(dev, kt, n, k):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_topk_scratch_bytes(dev._h, kt, n, k, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Call:
    """One input on the device and, per call, outputs of exactly k elements and a work buffer of exactly the reported bytes."""

    def __init__(self, dev, name, bits):
        self.dev, self.name, self.kt, self.bits = dev, name, BY_NAME[name][1], bits
        self.inp = Guarded(dev, bits, guard_bytes=SENTINELS * bits.dtype.itemsize, seed=5)

    def enqueue(self, order, k, work=None, fill=None, want_keys=True, want_index=True):
        bits, n = self.bits, self.bits.size
        wb = topk_bytes(self.dev, self.kt, n, k)
        ko = Guarded(self.dev, nbytes=k * bits.dtype.itemsize, guard_bytes=SENTINELS * bits.dtype.itemsize, seed=6) if want_keys else None
        io = Guarded(self.dev, nbytes=4 * k, guard_bytes=SENTINELS * 4, seed=7) if want_index else None
        own = work is None
        w = Guarded(self.dev, nbytes=wb, seed=8, fill=fill) if own else work
        assert w.nbytes >= wb
        rc = _lib.load().adlhip_topk_typed(self.dev._h, self.kt, order, self.inp.ptr(), n, k, ko.ptr() if ko else None,
                                           io.ptr() if io else None, w.ptr(), w.nbytes)
        assert rc == 0, lib_err()
        return ko, io, (w if own else None)

    def collect(self, order, k, ko, io, w, perm):
        """reads a call's outputs, checks every guard and the input, compares with perm[:k]; releases the call's buffers"""
        try:
            got_i = io.read(np.uint32) if io else None
            got_k = ko.read(self.bits.dtype) if ko else None
            if w is not None:
                w.check_guard()
            assert np.array_equal(self.inp.read(self.bits.dtype), self.bits), "top-k changed d_keys_in"
            want = perm[:k]
            if io:
                assert np.array_equal(got_i.astype(np.int64), want), \
                    "%s order %d n %d k %d: indices differ" % (self.name, order, self.bits.size, k)
            if ko:
                assert np.array_equal(got_k, self.bits[want]), "%s order %d n %d k %d: keys differ" % (self.name, order, self.bits.size, k)
        finally:
            for b in (ko, io, w):
                if b is not None:
                    b.release()

    def check(self, order, k, perm, **kw):
        ko, io, w = self.enqueue(order, k, **kw)
        self.collect(order, k, ko, io, w, perm)

    def release(self):
        self.inp.release()


def run_all(dev, name, bits, ks_of, orders=(ASC, DESC), algos=ALGOS):
    """ks_of(perm, order) -> the k values; both paths, idle state after each"""
    c = Call(dev, name, bits)
    try:
        for order in orders:
            perm = expected_perm(bits, name, order)
            for k in sorted(set(int(k) for k in ks_of(perm, order) if 0 <= k <= bits.size)):
                for algo in algos:
                    dev.setParam("topk.algo", algo)
                    c.check(order, k, perm)
                    assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.algo", -1)
        c.release()


def tie_ks(bits, perm):
    """for every tie group of the expected order: where it starts, starts + 1, ends - 1 (as counts k)"""
    s = bits[perm]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    ends = np.concatenate([starts[1:], [s.size]])
    ks = set()
    for a, b in zip(starts.tolist(), ends.tolist()):
        ks.update((a, a + 1, b - 1, b))
    return sorted(k for k in ks if 1 <= k <= s.size)


# ---------------------------------------------------------------------------------------------
# every type, both orders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_every_type_and_order_with_special_patterns(dev, name, kt, dt, udt, order):
    n = 100_003
    bits = random_bits(udt, n, seed=100 + kt)
    run_all(dev, name, bits, lambda perm, o: (1, 2, 1000, n - 1, n), orders=(order,))


# ---------------------------------------------------------------------------------------------
# tile and vector edges
# ---------------------------------------------------------------------------------------------
def _edge_sizes(w):
    t = TILE[w]
    return [1, 2, 3, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, (4 << 20) + 3]


# (the edges of both tiles for both types: a tile edge of the other width is still an odd size)
@pytest.mark.parametrize("n", sorted(set(_edge_sizes(4) + _edge_sizes(8))))
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_tile_and_vector_edges(dev, name, n):
    udt = BY_NAME[name][3]
    bits = random_bits(udt, n, seed=7 * n + 1)
    big = n > (1 << 20)
    # (the large size: one order per type, to stay within a few seconds; the small sizes take both)
    orders = (ASC, DESC) if not big else ((DESC,) if name == "f32" else (ASC,))
    run_all(dev, name, bits, lambda perm, o: (1, min(n, 7), n), orders=orders)


# ---------------------------------------------------------------------------------------------
# ties through the boundary
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "i64", "u32", "f64"])
def test_ties_keys_drawn_from_37_values(dev, name):
    udt = BY_NAME[name][3]
    bits = random_bits(udt, 20_011, seed=37, few=True)
    run_all(dev, name, bits, lambda perm, o: tie_ks(bits, perm)[:24] + tie_ks(bits, perm)[-8:])


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_ties_all_keys_equal(dev, name):
    udt = BY_NAME[name][3]
    n = (1 << 20) + 5   # more than one position digit
    bits = np.full(n, 0x3f800000 if udt is np.uint32 else 0xfffffffffffffff5, dtype=udt)
    c = Call(dev, name, bits)
    try:
        perm = np.arange(n, dtype=np.int64)   # selection runs on position digits alone: the indices are 0..k-1
        for order in (ASC, DESC):
            assert np.array_equal(expected_perm(bits[:1000], name, order), perm[:1000])
            for k in (1, 2, 2047, 2048, 2049, 4097, (1 << 11) * 300 + 1, n - 1, n):
                dev.setParam("topk.algo", 1)
                c.check(order, k, perm)
                assert dev.getParam("debug.idle_dirty") == 0
            dev.setParam("topk.algo", 0)
            c.check(order, 2049, perm)
    finally:
        dev.setParam("topk.algo", -1)
        c.release()


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_ties_one_value_fills_ninety_percent(dev, name):
    udt = BY_NAME[name][3]
    n = 50_021
    bits = random_bits(udt, n, seed=90)
    rng = np.random.default_rng(91)
    bits[rng.random(n) < 0.9] = bits[17]

    def ks(perm, order):
        s = bits[perm]
        inside = np.flatnonzero(s == bits[17])
        a, b = int(inside[0]), int(inside[-1]) + 1
        return (a, a + 1, (a + b) // 2, b - 1, b, min(b + 1, n))
    run_all(dev, name, bits, ks)


# ---------------------------------------------------------------------------------------------
# levels whose keys share one bucket
# ---------------------------------------------------------------------------------------------
def _one_bucket_inputs():
    rng = np.random.default_rng(55)
    n = 30_011
    out = []
    for name in ("u32", "f32", "i64", "f64"):
        udt = BY_NAME[name][3]
        w = np.dtype(udt).itemsize
        base = udt(0x3f9d70a4 if w == 4 else 0x3ff3ae147ae147ae)
        low = rng.integers(0, 256, size=n).astype(udt)
        out.append((name + "-lowest-byte", name, (base & ~udt(0xff)) | low))
        out.append((name + "-highest-byte", name, (base & udt((1 << (8 * w - 8)) - 1)) | (low << udt(8 * w - 8))))
    for name in ("i64", "f64"):
        d = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
        out.append((name + "-high-dword", name, (d << np.uint64(32)) | np.uint64(0x89abcdef)))
        out.append((name + "-low-dword", name, np.uint64(0x40091eb800000000) | d))
    for name in ("f32", "i64"):
        udt = BY_NAME[name][3]
        x = random_bits(udt, n, seed=56)
        asc = x[expected_perm(x, name, ASC)]
        out.append((name + "-sorted-ascending", name, np.ascontiguousarray(asc)))
        out.append((name + "-sorted-descending", name, np.ascontiguousarray(asc[::-1])))
    return out


_ONE_BUCKET = _one_bucket_inputs()


@pytest.mark.parametrize("case", _ONE_BUCKET, ids=[c[0] for c in _ONE_BUCKET])
def test_one_bucket_levels_and_sorted_inputs(dev, case):
    _, name, bits = case
    n = bits.size
    run_all(dev, name, bits, lambda perm, o: (1, 100, n // 2, n))


# ---------------------------------------------------------------------------------------------
# survivor hand-off: how many keys the chosen bin of level 0 holds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("held", [1, 4096, 4097, "all"])
def test_survivor_hand_off(dev, held):
    """u32 keys, ascending and descending: `held` keys carry the top digit (11 bits) 1000, the k-th key among them"""
    rng = np.random.default_rng(77)
    n = 40_009
    m = n if held == "all" else held
    inside = (np.uint32(1000) << np.uint32(21)) | rng.integers(0, 1 << 21, size=m, dtype=np.uint32)
    rest = n - m
    below = (rng.integers(0, 1000, size=rest // 2).astype(np.uint32) << np.uint32(21)) | rng.integers(0, 1 << 21, size=rest // 2, dtype=np.uint32)
    above = (rng.integers(1001, 2048, size=rest - rest // 2).astype(np.uint32) << np.uint32(21)) | \
        rng.integers(0, 1 << 21, size=rest - rest // 2, dtype=np.uint32)
    bits = np.concatenate([inside, below, above]).astype(np.uint32)
    rng.shuffle(bits)

    def ks(perm, order):
        s = bits[perm] >> np.uint32(21)
        at = np.flatnonzero(s == 1000)
        a, b = int(at[0]), int(at[-1]) + 1
        assert b - a == m
        return (a + 1, (a + b + 1) // 2, b)
    run_all(dev, "u32", bits, ks)


# ---------------------------------------------------------------------------------------------
# the work buffer's contents on entry do not matter; call sequences
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    n, k = 70_001, 777
    bits = random_bits(np.uint32, n, seed=31, few=True)
    other = random_bits(np.uint32, n, seed=32)
    c, c2 = Call(dev, "f32", bits), Call(dev, "f32", other)
    try:
        perm = expected_perm(bits, "f32", DESC)
        perm2 = expected_perm(other, "f32", ASC)
        for algo in ALGOS:
            dev.setParam("topk.algo", algo)
            for fill in (0x00, 0xff):
                c.check(DESC, k, perm, fill=fill)
            # left over from a different call: same size class, other keys, other order, other k
            wb = max(topk_bytes(dev, 2, n, k), topk_bytes(dev, 2, n, 5000))
            w = Guarded(dev, nbytes=wb, seed=9)
            try:
                ko, io, _ = c2.enqueue(ASC, 5000, work=w)
                c2.collect(ASC, 5000, ko, io, None, perm2)
                ko, io, _ = c.enqueue(DESC, k, work=w)
                c.collect(DESC, k, ko, io, None, perm)
                w.check_guard()
            finally:
                w.release()
            assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.algo", -1)
        c.release()
        c2.release()


def test_call_sequences(dev):
    n = 90_001
    a_bits = random_bits(np.uint64, n, seed=41)
    b_bits = random_bits(np.uint32, n, seed=42, few=True)
    a, b = Call(dev, "f64", a_bits), Call(dev, "i32", b_bits)
    p = Pprims()
    sort_buf = None
    try:
        pa, pb = expected_perm(a_bits, "f64", DESC), expected_perm(b_bits, "i32", ASC)
        for algo in ALGOS:
            dev.setParam("topk.algo", algo)
            # two different top-k calls back to back, nothing waits between them
            ra = a.enqueue(DESC, 333)
            rb = b.enqueue(ASC, 4099)
            a.collect(DESC, 333, *ra, pa)
            b.collect(ASC, 4099, *rb, pb)
            # a top-k between two sorts on the same handle
            keys = np.random.default_rng(43).integers(0, 1 << 32, size=n, dtype=np.uint32)
            sort_buf = Buffer(dev, n, np.uint32)
            sort_buf.write(keys)
            p.radixSort(dev, sort_buf, n)
            rb = b.enqueue(ASC, 12, want_keys=False)
            first = sort_buf.toHost()
            sort_buf.write(keys[::-1].copy())
            p.radixSort(dev, sort_buf, n)
            assert np.array_equal(first, np.sort(keys)) and np.array_equal(sort_buf.toHost(), np.sort(keys))
            b.collect(ASC, 12, *rb, pb)
            ra = a.enqueue(DESC, 50, want_index=False)   # keys only
            a.collect(DESC, 50, *ra, pa)
            sort_buf.release()
            sort_buf = None
            assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.algo", -1)
        if sort_buf is not None:
            sort_buf.release()
        p.close()
        a.release()
        b.release()


def test_default_picks_by_k_and_the_knob_round_trips(dev):
    assert dev.getParam("topk.algo") == -1
    n = 33_333
    bits = random_bits(np.uint32, n, seed=61)
    run_all(dev, "i32", bits, lambda perm, o: (n // 8, n // 8 + 1), algos=(-1,))
    for v in (0, 1, -1):
        dev.setParam("topk.algo", v)
        assert dev.getParam("topk.algo") == v
    with pytest.raises(Exception):
        dev.setParam("topk.algo", 2)
    assert dev.getParam("topk.algo") == -1


def test_scratch_bytes_stay_within_the_documented_bound(dev):
    """at most the argsort's work for n + n (4 + key bytes) + the k-element finish's own scratch (its partner array, its gathered keys,
    the larger of its two sorts' work), each part rounded up to 256 bytes"""
    lib = _lib.load()

    def w_argsort(kt, m):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_sort_typed_scratch_bytes(dev._h, kt, 2, 0, m, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib_err()
        return c.value

    def w_u32(m):
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_radix_sort_scratch_bytes(dev._h, 0, m, ctypes.byref(a), ctypes.byref(b)) == 0, lib_err()
        return b.value

    def up(x):
        return (x + 255) // 256 * 256

    for name in ("f32", "i64"):
        kt, kb = BY_NAME[name][1], np.dtype(BY_NAME[name][3]).itemsize
        for n in (100_003, (1 << 20) + 5, (4 << 20) + 3):
            for k in (1, 1000, n // 8, n):
                finish = up(4 * k) + up(kb * k) + max(w_u32(k), w_argsort(kt, k))
                bound = up(w_argsort(kt, n)) + up(n * kb) + up(4 * n) + finish
                got = topk_bytes(dev, kt, n, k)
                print("%s n %d k %d: %d bytes, bound %d" % (name, n, k, got, bound))
                assert got <= bound, (name, n, k)


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32 = 2
    n, k = 5000, 100
    bits = random_bits(np.uint32, n, seed=71)
    wb = topk_bytes(dev, F32, n, k)
    inp = Guarded(dev, bits, seed=1)
    marks_k = np.arange(k, dtype=np.uint32) ^ np.uint32(0xa5a5a5a5)
    marks_i = np.arange(k, dtype=np.uint32) ^ np.uint32(0x5a5a5a5a)
    ko = Guarded(dev, marks_k, guard_bytes=SENTINELS * 4, seed=2)
    io = Guarded(dev, marks_i, guard_bytes=SENTINELS * 4, seed=3)
    w = Guarded(dev, nbytes=wb, seed=4)
    sz = ctypes.c_size_t()

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    try:
        for algo in ALGOS:
            dev.setParam("topk.algo", algo)
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, n + 1, ko.ptr(), io.ptr(), w.ptr(), wb), "k > n")
            refused(lib.adlhip_topk_scratch_bytes(dev._h, F32, n, n + 1, ctypes.byref(sz)), "scratch, k > n")
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, k, None, None, w.ptr(), wb), "both outputs null")
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, k - 1, ko.ptr(4), io.ptr(), w.ptr(), wb), "misaligned keys out")
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, k - 1, ko.ptr(), io.ptr(4), w.ptr(), wb), "misaligned index out")
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(4), n - 1, k, ko.ptr(), io.ptr(), w.ptr(), wb), "misaligned input")
            assert str(wb) in refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, k, ko.ptr(), io.ptr(), w.ptr(), wb - 1),
                                      "work one byte short")
            refused(lib.adlhip_topk_typed(dev._h, F32, ASC, inp.ptr(), n, k, inp.ptr(16), io.ptr(), w.ptr(), wb), "output overlaps the input")
            for bad in (-1, 6, 99):
                refused(lib.adlhip_topk_typed(dev._h, bad, ASC, inp.ptr(), n, k, ko.ptr(), io.ptr(), w.ptr(), wb), "key_type %d" % bad)
                refused(lib.adlhip_topk_scratch_bytes(dev._h, bad, n, k, ctypes.byref(sz)), "scratch, key_type %d" % bad)
            for bad in (-1, 2):
                refused(lib.adlhip_topk_typed(dev._h, F32, bad, inp.ptr(), n, k, ko.ptr(), io.ptr(), w.ptr(), wb), "order %d" % bad)
            # k == 0 and n == 0 succeed and enqueue nothing
            assert lib.adlhip_topk_typed(dev._h, F32, DESC, inp.ptr(), n, 0, ko.ptr(), io.ptr(), w.ptr(), wb) == 0, lib_err()
            assert lib.adlhip_topk_typed(dev._h, F32, DESC, None, 0, 0, None, None, None, 0) == 0, lib_err()
            assert np.array_equal(ko.read(np.uint32), marks_k) and np.array_equal(io.read(np.uint32), marks_i)
            assert np.array_equal(inp.read(np.uint32), bits)
            w.check_guard()
            assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.algo", -1)
        for b in (inp, ko, io, w):
            b.release()


# ---------------------------------------------------------------------------------------------
# Python mirror and torch front end
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    n, k = 60_007, 500
    bits = random_bits(np.uint64, n, seed=81)
    p = Pprims()
    keys = Buffer(dev, n, np.float64)
    kout = Buffer(dev, k, np.float64)
    try:
        keys.write(bits.view(np.float64))
        out = p.topk(dev, keys, n, k, descending=True, keysOut=kout)
        want = expected_perm(bits, "f64", DESC)[:k]
        assert out.getSize() == k and np.array_equal(out.toHost().astype(np.int64), want)
        assert np.array_equal(kout.toHost().view(np.uint64), bits[want])
        out.release()
        out = p.topk(dev, keys, n, 0)
        assert out.getSize() == 0
        out.release()
    finally:
        keys.release()
        kout.release()
        p.close()


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
        return torch.where(t == 0, torch.ones_like(t), t)   # no -0 (and no +0 either), no NaN
    return torch.randint(-500, 500, (n,), dtype=dtype, device="cuda", generator=g)   # many ties


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_topk_matches_torch(sorter, dtype_name, largest):
    import torch
    dtype = getattr(torch, dtype_name)
    n = 100_003
    t = _torch_input(torch, dtype, n)
    keep = t.clone()
    order = torch.sort(t, descending=largest, stable=True).indices
    for k in (1, 10, 1000, n // 8 + 1, n):
        values, indices = sorter.topk(t, k, largest=largest)
        torch.cuda.synchronize()
        assert values.dtype == dtype and indices.dtype == torch.int64 and values.shape == (k,) and indices.shape == (k,)
        assert torch.equal(values, torch.topk(t, k, largest=largest, sorted=True).values)
        assert torch.equal(indices, order[:k])
    values, indices = sorter.topk(t, 10, largest=largest, sorted=False)   # accepted; the output is sorted all the same
    assert torch.equal(indices, order[:10])
    assert torch.equal(t, keep), "the input was changed"
    half = t[::2]   # a strided view
    assert not half.is_contiguous()
    values, indices = sorter.topk(half, 100, largest=largest)
    assert torch.equal(values, torch.topk(half, 100, largest=largest).values)
    assert torch.equal(indices, torch.sort(half, descending=largest, stable=True).indices[:100])
    for view in (t[1:], t[3:]):   # contiguous views that start at an odd offset (the ABI wants 16-byte alignment)
        assert view.is_contiguous() and view.data_ptr() % 16
        view_order = torch.sort(view, descending=largest, stable=True).indices
        for k in (1, 100, view.numel()):
            values, indices = sorter.topk(view, k, largest=largest)
            assert torch.equal(values, torch.topk(view, k, largest=largest, sorted=True).values)
            assert torch.equal(indices, view_order[:k])
    values, indices = sorter.topk(t[1:1], 0, largest=largest)   # empty, at an odd offset
    assert values.numel() == 0 and indices.numel() == 0 and indices.dtype == torch.int64 and values.dtype == dtype
    with pytest.raises(ValueError):
        sorter.topk(t[1:1], 1)
    assert torch.equal(t, keep), "the input was changed"
    values, indices = sorter.topk(t, 0, largest=largest)
    assert values.numel() == 0 and indices.numel() == 0 and indices.dtype == torch.int64 and values.dtype == dtype
    with pytest.raises(ValueError):
        sorter.topk(t, n + 1)
    with pytest.raises(ValueError):
        sorter.topk(t, -1)


def test_torch_sorter_topk_is_bound_to_its_stream(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.arange(100, dtype=torch.int32, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "topk", boom)
        with pytest.raises(RuntimeError):
            sorter.topk(t, 3)
        monkeypatch.undo()
    values, indices = sorter.topk(t, 3)
    assert values.tolist() == [99, 98, 97] and indices.tolist() == [99, 98, 97]
    for bad in (torch.zeros(8, dtype=torch.float16, device="cuda"), torch.zeros((4, 4), dtype=torch.float32, device="cuda"), [3.0, 1.0]):
        with pytest.raises((TypeError, ValueError)):
            sorter.topk(bad, 1)
