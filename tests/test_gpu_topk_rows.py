"""Row-wise top-k on the GPU (include/adlhip.h adlhip_topk_rows_typed; oclradixsort_amd/csrc/toprows_kernels.hpp;
TorchSorter.topk_rows).

The expected output is stated independently of the key codec, as in test_gpu_topk.py: a key's ordinal is its bit pattern read as
sign-magnitude for floats, the value itself for integers; per row the expected permutation is the stable argsort of the ordinal
(descending: of the negated ordinal), truncated to k.  Everything is compared bit for bit, nothing is excluded, there is no tolerance.

Every device buffer carries guard bytes behind its payload, checked after each call: the input, both outputs (sized exactly
rows * k) and the work buffer (sized exactly the reported bytes).  The input is compared with its original afterwards.  Unless a
test says otherwise a case runs under "topk.rows_algo" = 1 (the row kernel) and = 0 (the per-row loop), each result is compared with
numpy and the two with each other, and "debug.idle_dirty" is 0 after every call.

CAP below is the number of composites a workgroup of the row kernel holds in LDS (4096); KMAX the largest k it serves (2048).
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, _lib

pytestmark = pytest.mark.gpu

ASC, DESC = 0, 1
TYPES = [("u32", 0, np.uint32, np.uint32), ("i32", 1, np.int32, np.uint32), ("f32", 2, np.float32, np.uint32),
         ("u64", 3, np.uint64, np.uint64), ("i64", 4, np.int64, np.uint64), ("f64", 5, np.float64, np.uint64)]
BY_NAME = {t[0]: t for t in TYPES}
TYPE_IDS = [t[0] for t in TYPES]
ORDER_IDS = ["asc", "desc"]
SENTINELS = 64
ALGOS = (1, 0)   # "topk.rows_algo": the row kernel, the per-row loop
CAP, KMAX = 4096, 2048

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
# the expected order, from numpy (the helper lines of test_gpu_topk.py)
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
def _reset(d):
    d.setParam("topk.rows_algo", -1)
    d.setParam("debug.topk_rows_grid", 0)
    d.setParam("topk.algo", -1)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    _reset(d)
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


def rows_bytes(dev, kt, rows, cols, k):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_topk_rows_scratch_bytes(dev._h, kt, rows, cols, k, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Matrix:
    """rows x cols keys at a row stride on the device (flat: (rows - 1) * stride + cols elements, nothing behind the last row but the
    guard) and, per order, every row's expected permutation (computed once)."""

    def __init__(self, dev, name, flat, rows, cols, stride=None):
        self.dev, self.name, self.kt = dev, name, BY_NAME[name][1]
        self.rows, self.cols, self.stride = rows, cols, cols if stride is None else stride
        assert flat.size == (rows - 1) * self.stride + cols
        self.flat = flat
        self.inp = Guarded(dev, flat, guard_bytes=SENTINELS * flat.dtype.itemsize, seed=5)
        self._perm = {}

    def row(self, r):
        return self.flat[r * self.stride:r * self.stride + self.cols]

    def perms(self, order):
        if order not in self._perm:
            self._perm[order] = [expected_perm(self.row(r), self.name, order) for r in range(self.rows)]
        return self._perm[order]

    def expected(self, order, k):
        p = self.perms(order)
        idx = np.stack([p[r][:k] for r in range(self.rows)]).astype(np.int64)
        keys = np.stack([self.row(r)[p[r][:k]] for r in range(self.rows)])
        return idx, keys

    def enqueue(self, order, k, work=None, fill=None, want_keys=True, want_index=True):
        w_item = self.flat.dtype.itemsize
        wb = rows_bytes(self.dev, self.kt, self.rows, self.cols, k)
        nk = self.rows * k
        ko = Guarded(self.dev, nbytes=nk * w_item, guard_bytes=SENTINELS * w_item, seed=6) if want_keys else None
        io = Guarded(self.dev, nbytes=4 * nk, guard_bytes=SENTINELS * 4, seed=7) if want_index else None
        own = work is None
        w = Guarded(self.dev, nbytes=wb, seed=8, fill=fill) if own else work
        assert w.nbytes >= wb
        rc = _lib.load().adlhip_topk_rows_typed(self.dev._h, self.kt, order, self.inp.ptr(), self.rows, self.cols, self.stride, k,
                                                ko.ptr() if ko else None, io.ptr() if io else None, w.ptr(), w.nbytes)
        assert rc == 0, lib_err()
        return ko, io, (w if own else None)

    def collect(self, order, k, ko, io, w):
        """reads a call's outputs, checks every guard and the input, compares with numpy; releases the call's buffers; returns
        (indices, keys) as read"""
        try:
            got_i = io.read(np.uint32).reshape(self.rows, k) if io else None
            got_k = ko.read(self.flat.dtype).reshape(self.rows, k) if ko else None
            if w is not None:
                w.check_guard()
            assert np.array_equal(self.inp.read(self.flat.dtype), self.flat), "top-k of rows changed d_keys_in"
            want_i, want_k = self.expected(order, k)
            what = "%s order %d rows %d cols %d stride %d k %d" % (self.name, order, self.rows, self.cols, self.stride, k)
            if io:
                bad = np.flatnonzero((got_i.astype(np.int64) != want_i).any(axis=1))
                assert bad.size == 0, "%s: columns differ in rows %s" % (what, bad[:8].tolist())
            if ko:
                bad = np.flatnonzero((got_k != want_k).any(axis=1))
                assert bad.size == 0, "%s: keys differ in rows %s" % (what, bad[:8].tolist())
            return got_i, got_k
        finally:
            for b in (ko, io, w):
                if b is not None:
                    b.release()

    def check(self, order, k, algos=ALGOS, **kw):
        """one (order, k) under every algo: numpy, the guards, the input, the idle state; the algos against each other"""
        seen = []
        try:
            for algo in algos:
                self.dev.setParam("topk.rows_algo", algo)
                ko, io, w = self.enqueue(order, k, **kw)
                seen.append(self.collect(order, k, ko, io, w))
                assert self.dev.getParam("debug.idle_dirty") == 0
        finally:
            self.dev.setParam("topk.rows_algo", -1)
        for other in seen[1:]:
            for a, b in zip(seen[0], other):
                assert (a is None and b is None) or np.array_equal(a, b), "the two paths disagree"

    def release(self):
        self.inp.release()


def make_matrix(dev, name, rows, cols, seed, stride=None, few=False):
    """every row has different data (and its own share of the special patterns)"""
    udt = BY_NAME[name][3]
    stride = cols if stride is None else stride
    flat = np.concatenate([random_bits(udt, stride, seed + 1000 * r, few=few) for r in range(rows)])[:(rows - 1) * stride + cols]
    return Matrix(dev, name, np.ascontiguousarray(flat), rows, cols, stride)


# ---------------------------------------------------------------------------------------------
# 1. every type, both orders, special bit patterns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=ORDER_IDS)
@pytest.mark.parametrize("name,kt,dt,udt", TYPES, ids=TYPE_IDS)
def test_every_type_and_order_with_special_patterns(dev, name, kt, dt, udt, order):
    for cols in (1000, 5000):
        m = make_matrix(dev, name, 3, cols, seed=100 + kt + cols)
        try:
            for r in range(3):   # the special patterns are in every row
                assert np.isin(SPECIALS[np.dtype(udt).itemsize], m.row(r)).all()
            for k in (1, 10):
                m.check(order, k)
        finally:
            m.release()


# ---------------------------------------------------------------------------------------------
# 2. edge sizes; row_stride == cols and 7 rows, so most rows start off a 16-byte boundary
# ---------------------------------------------------------------------------------------------
EDGE_COLS = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 8191, 8193, 16387, 100003]
EDGE_KS = [1, 2, 63, 64, 65, 2047, 2048]


@pytest.mark.parametrize("cols", EDGE_COLS)
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_edge_sizes(dev, name, cols):
    ks = [k for k in EDGE_KS if k <= cols]
    if cols <= KMAX and cols not in ks:
        ks.append(cols)
    m = make_matrix(dev, name, 7, cols, seed=7 * cols + 1)
    try:
        for order in (ASC, DESC):
            for k in ks:
                m.check(order, k)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------
# 3. padding between the rows: keys that would win in either order, never to be seen in the output
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1000, 5000])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_padding_between_rows_is_not_read(dev, name, cols):
    udt = BY_NAME[name][3]
    rows, stride = 5, cols + 5
    flat = random_bits(udt, (rows - 1) * stride + cols, seed=300 + cols)
    ones = udt(0xffffffff if udt is np.uint32 else 0xffffffffffffffff)
    for r in range(rows - 1):
        pad = np.array([0, ones, 0, ones, 0] if r % 2 == 0 else [ones, 0, ones, 0, ones], dtype=udt)   # alternating
        flat[r * stride + cols:(r + 1) * stride] = pad
    m = Matrix(dev, name, flat, rows, cols, stride)
    try:
        for order in (ASC, DESC):
            for k in (1, 10, 1000):
                m.check(order, k)   # (numpy's expectation is built from the cols keys of each row alone)
                want_i, _ = m.expected(order, k)
                assert want_i.max() < cols
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------
# 4. the row loop of the kernel: few workgroups take many rows in turns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_three_workgroups_take_ten_rows(dev, name):
    dev.setParam("debug.topk_rows_grid", 3)
    try:
        assert dev.getParam("debug.topk_rows_grid") == 3
        for cols in (777, 5001):
            m = make_matrix(dev, name, 10, cols, seed=400 + cols)
            try:
                for order in (ASC, DESC):
                    m.check(order, 33)
            finally:
                m.release()
    finally:
        dev.setParam("debug.topk_rows_grid", 0)
    with pytest.raises(Exception):
        dev.setParam("debug.topk_rows_grid", -1)
    assert dev.getParam("debug.topk_rows_grid") == 0


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_a_single_row(dev, name):
    for cols in (1000, 20_011):
        m = make_matrix(dev, name, 1, cols, seed=410 + cols)
        try:
            for order in (ASC, DESC):
                m.check(order, 100)
        finally:
            m.release()


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_three_hundred_rows_of_4097(dev, name):
    m = make_matrix(dev, name, 300, 4097, seed=420)
    try:
        m.check(DESC if name == "f32" else ASC, 50)
        m.check(ASC if name == "f32" else DESC, 1, algos=(1,))
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------
# 5. ties through the boundary
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_ties_every_key_of_a_row_equal(dev, name):
    """every key level keeps everything; the position digits decide: the columns are 0 .. k-1"""
    udt = BY_NAME[name][3]
    rows, cols, k = 2, 100_003, 100
    flat = np.empty(rows * cols, dtype=udt)
    flat[:cols] = 0x3f800000 if udt is np.uint32 else 0xfffffffffffffff5
    flat[cols:] = 0xbf800001 if udt is np.uint32 else 0x0000000000000005
    m = Matrix(dev, name, flat, rows, cols)
    try:
        for order in (ASC, DESC):
            assert np.array_equal(m.expected(order, k)[0], np.tile(np.arange(k), (rows, 1)))
            m.check(order, k)
            m.check(order, KMAX, algos=(1,))
    finally:
        m.release()


@pytest.mark.parametrize("name", ["f32", "i64", "u32", "f64"])
def test_ties_keys_drawn_from_37_values(dev, name):
    m = make_matrix(dev, name, 3, 20_011, seed=37, few=True)
    try:
        for order in (ASC, DESC):
            p = m.perms(order)[0]
            s = m.row(0)[p]
            starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))   # where row 0's tie groups begin
            ks = sorted(set(int(k) for a in starts[:4] for k in (a, a + 1, a - 1) if 1 <= k <= KMAX))
            assert len(ks) >= 6
            for k in ks:
                m.check(order, k)
    finally:
        m.release()


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_rows_already_sorted_and_reverse_sorted(dev, name):
    udt = BY_NAME[name][3]
    cols = 30_011
    x = random_bits(udt, cols, seed=56)
    asc = x[expected_perm(x, name, ASC)]
    flat = np.concatenate([asc, asc[::-1]]).astype(udt)
    m = Matrix(dev, name, flat, 2, cols)
    try:
        for order in (ASC, DESC):
            for k in (1, 100, KMAX):
                m.check(order, k)
    finally:
        m.release()


def test_u64_keys_whose_high_dwords_are_all_equal(dev):
    rng = np.random.default_rng(57)
    cols = 30_011
    low = rng.integers(0, 1 << 32, size=3 * cols, dtype=np.uint64)
    low[rng.integers(0, 3 * cols, size=cols)] = 0x89abcdef   # and ties among them
    flat = np.uint64(0x40091eb800000000) | low
    for name in ("u64", "i64", "f64"):
        m = Matrix(dev, name, flat, 3, cols)
        try:
            for order in (ASC, DESC):
                for k in (1, 100, KMAX):
                    m.check(order, k)
        finally:
            m.release()


# ---------------------------------------------------------------------------------------------
# 6. hand-off boundaries: u32 ascending (the code is the key), cols = 8192, k = 2048
# ---------------------------------------------------------------------------------------------
def levels_taken(row, k):
    """numpy model of the select form's level rule for u32 ascending keys: [(S, C)] per level taken, S = items certainly selected,
    C = population of the chosen bin; it stops at the first level with S + C <= CAP.  Digits: 11, 11, 10 key bits, then the position
    bits of cols, 11 at a time."""
    cols = row.size
    pos_bits = max(1, int(cols - 1).bit_length())
    plan = [(0, 21, 11), (0, 10, 11), (0, 0, 10)]
    left = pos_bits
    while left > 0:
        bits = min(left, 11)
        plan.append((1, left - bits, bits))
        left -= bits
    alive = np.ones(cols, bool)
    pos = np.arange(cols, dtype=np.int64)
    want, before, out = k, 0, []
    for from_pos, shift, bits in plan:
        dg = ((pos if from_pos else row.astype(np.int64)) >> shift) & ((1 << bits) - 1)
        hist = np.bincount(dg[alive], minlength=1 << bits)
        cum = np.cumsum(hist)
        b = int(np.searchsorted(cum, want))   # first bin with cum >= want
        skip = int(cum[b] - hist[b])
        before += skip
        want -= skip
        alive &= dg == b
        out.append((before, int(hist[b])))
        if before + hist[b] <= CAP:
            return out, len(plan)
    raise AssertionError("the last level holds one composite per bin")


def _handoff_row(kind, rng):
    cols = 8192
    d = np.uint32(21)

    def with_top(digits, n):
        return (np.asarray(digits, dtype=np.uint32) << d) | rng.integers(0, 1 << 21, size=n, dtype=np.uint32)

    if kind in ("fits-exactly", "one-too-many"):
        held = 3096 if kind == "fits-exactly" else 3097
        first = rng.choice(1 << 21, size=1000, replace=False).astype(np.uint32)   # 1000 distinct keys, top digit 0
        rest = cols - 1000 - held
        row = np.concatenate([first, with_top(np.ones(held), held), with_top(rng.integers(2, 2048, size=rest), rest)])
    elif kind == "bin-equals-rank":
        # level 0: 1000 before, 5000 in the chosen bin (too many); level 1 inside it: 500 before, 548 in the chosen bin = the rank wanted
        first = rng.choice(1 << 21, size=1000, replace=False).astype(np.uint32)
        second = np.concatenate([np.zeros(500), np.full(548, 5), rng.integers(6, 2048, size=3952)]).astype(np.uint32)
        inside = (np.uint32(1) << d) | (second << np.uint32(10)) | rng.integers(0, 1 << 10, size=5000, dtype=np.uint32)
        rest = cols - 6000
        row = np.concatenate([first, inside, with_top(rng.integers(2, 2048, size=rest), rest)])
    else:   # "position-levels": every key equal
        return np.full(cols, 0x12345678, dtype=np.uint32)
    row = row.astype(np.uint32)
    rng.shuffle(row)
    return row


@pytest.mark.parametrize("kind", ["fits-exactly", "one-too-many", "bin-equals-rank", "position-levels"])
def test_hand_off_boundaries(dev, kind):
    """fits-exactly: S + C == CAP at level 0, the collect follows it.  one-too-many: S + C == CAP + 1, one more level.
    bin-equals-rank: the chosen bin of level 1 holds exactly the rank still wanted and is taken whole.
    position-levels: every key equal, so all three key levels keep the whole row and the position digits decide.  With cols = 8192
    there are two position levels (11 + 2 bits) and selection stops at the first of them: a bin of the level before the last holds at
    most 2^11 columns and S < k <= KMAX, so S + C <= CAP there for every input longer than CAP -- the last level is the rule's safety
    net and no row can reach it.  The model below states how far each row goes."""
    rng = np.random.default_rng(600)
    k = KMAX
    rows = [_handoff_row(kind, rng), _handoff_row(kind, rng)]
    for row in rows:
        taken, levels = levels_taken(row, k)
        if kind == "fits-exactly":
            assert taken == [(1000, 3096)] and sum(taken[0]) == CAP
        elif kind == "one-too-many":
            assert taken[0] == (1000, 3097) and len(taken) == 2
        elif kind == "bin-equals-rank":
            assert taken == [(1000, 5000), (1500, 548)] and k - 1500 == 548
        else:
            assert levels == 5 and taken == [(0, 8192)] * 3 + [(2044, 4)]
    m = Matrix(dev, "u32", np.concatenate(rows), 2, 8192)
    try:
        m.check(ASC, k)
    finally:
        m.release()


# ---------------------------------------------------------------------------------------------
# 7. the default rule and the fallback
# ---------------------------------------------------------------------------------------------
def test_k_above_the_row_kernels_limit(dev):
    lib = _lib.load()
    rows, cols, k = 3, 5000, KMAX + 1
    m = make_matrix(dev, "f32", rows, cols, seed=700)
    marks_k = np.arange(rows * k, dtype=np.uint32) ^ np.uint32(0xa5a5a5a5)
    marks_i = np.arange(rows * k, dtype=np.uint32) ^ np.uint32(0x5a5a5a5a)
    ko = Guarded(dev, marks_k, guard_bytes=SENTINELS * 4, seed=2)
    io = Guarded(dev, marks_i, guard_bytes=SENTINELS * 4, seed=3)
    wb = rows_bytes(dev, m.kt, rows, cols, k)
    w = Guarded(dev, nbytes=wb, seed=4)
    try:
        dev.setParam("topk.rows_algo", 1)
        assert dev.getParam("topk.rows_algo") == 1
        rc = lib.adlhip_topk_rows_typed(dev._h, m.kt, DESC, m.inp.ptr(), rows, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb)
        assert rc == 1 and "2048" in lib_err(), lib_err()
        assert np.array_equal(ko.read(np.uint32), marks_k) and np.array_equal(io.read(np.uint32), marks_i)   # nothing was enqueued
        w.check_guard()
        assert dev.getParam("debug.idle_dirty") == 0
        dev.setParam("topk.rows_algo", -1)
        assert dev.getParam("topk.rows_algo") == -1
        for order in (ASC, DESC):
            m.check(order, k, algos=(-1,))     # by the loop
            m.check(order, KMAX, algos=(-1,))  # by the row kernel
        with pytest.raises(Exception):
            dev.setParam("topk.rows_algo", 2)
        assert dev.getParam("topk.rows_algo") == -1
    finally:
        dev.setParam("topk.rows_algo", -1)
        for b in (ko, io, w):
            b.release()
        m.release()


# ---------------------------------------------------------------------------------------------
# 8. the row kernel does not touch the work buffer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1000, 20_011])
def test_row_kernel_leaves_the_work_buffer_alone(dev, cols):
    m = make_matrix(dev, "i64", 5, cols, seed=800 + cols)
    k = 100
    wb = rows_bytes(dev, m.kt, 5, cols, k)
    w = Guarded(dev, nbytes=wb, seed=9, fill=0x5a)
    try:
        dev.setParam("topk.rows_algo", 1)
        ko, io, _ = m.enqueue(DESC, k, work=w)
        m.collect(DESC, k, ko, io, None)
        after = w.read(np.uint8)
        assert after.size == wb and (after == 0x5a).all(), "the row kernel wrote to d_work"
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("topk.rows_algo", -1)
        w.release()
        m.release()


# ---------------------------------------------------------------------------------------------
# 9. call sequences
# ---------------------------------------------------------------------------------------------
def _sort_keys_bytes(d, kt, n):
    a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = _lib.load().adlhip_sort_typed_scratch_bytes(d._h, kt, 0, 0, n, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    assert rc == 0, lib_err()
    return a.value, c.value


@pytest.mark.parametrize("algo", ALGOS, ids=["kernel", "loop"])
def test_a_rows_call_between_two_sorts(dev, algo):
    """sort, top-k of rows, sort on one handle and one scratch, nothing waits in between: the same three results as each gives on a
    fresh handle"""
    lib = _lib.load()
    F32 = 2
    n, rows, cols, k = 90_001, 6, 9001, 77
    a_bits = random_bits(np.uint32, n, seed=91)
    b_bits = random_bits(np.uint32, n, seed=92, few=True)
    flat = random_bits(np.uint32, rows * cols, seed=93)

    def run(d_sort1, d_rows, d_sort2):
        """each step on its handle; the steps share `work` when the handles are one"""
        one = d_sort1 is d_rows
        bufs = []
        try:
            tb, swb = _sort_keys_bytes(d_sort1, F32, n)
            rwb = rows_bytes(d_rows, F32, rows, cols, k)
            works = {}
            for d in (d_sort1, d_rows, d_sort2):
                if id(d) not in works:
                    works[id(d)] = Guarded(d, nbytes=max(swb, rwb), seed=10)
                    bufs.append(works[id(d)])
            ka, kb = Guarded(d_sort1, a_bits, seed=11), Guarded(d_sort2, b_bits, seed=12)
            tmp1, tmp2 = Guarded(d_sort1, nbytes=tb, seed=13), Guarded(d_sort2, nbytes=tb, seed=14)
            m = Matrix(d_rows, "f32", flat, rows, cols)
            bufs += [ka, kb, tmp1, tmp2]
            d_rows.setParam("topk.rows_algo", algo)
            w = works[id(d_sort1)]
            assert lib.adlhip_sort_keys_typed(d_sort1._h, F32, ASC, ka.ptr(), tmp1.ptr(), w.ptr(), w.nbytes, n) == 0, lib_err()
            ko, io, _ = m.enqueue(DESC, k, work=works[id(d_rows)])
            w = works[id(d_sort2)]
            assert lib.adlhip_sort_keys_typed(d_sort2._h, F32, DESC, kb.ptr(), tmp2.ptr(), w.ptr(), w.nbytes, n) == 0, lib_err()
            try:
                got_i, got_k = m.collect(DESC, k, ko, io, None)
            finally:
                m.release()
            out = (ka.read(np.uint32).copy(), got_i, got_k, kb.read(np.uint32).copy())
            for d in set((d_sort1, d_rows, d_sort2)):
                assert d.getParam("debug.idle_dirty") == 0
            assert one or len(works) == 3
            return out
        finally:
            d_rows.setParam("topk.rows_algo", -1)
            for b in bufs:
                b.release()

    fresh = [DeviceUtils.allocate() for _ in range(3)]
    try:
        apart = run(*fresh)
    finally:
        for d in fresh:
            DeviceUtils.deallocate(d)
    together = run(dev, dev, dev)
    assert np.array_equal(apart[0], a_bits[expected_perm(a_bits, "f32", ASC)])
    assert np.array_equal(apart[3], b_bits[expected_perm(b_bits, "f32", DESC)])
    for x, y in zip(apart, together):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32 = 2
    rows, cols, k = 4, 5000, 100
    flat = random_bits(np.uint32, rows * cols, seed=71)
    wb = rows_bytes(dev, F32, rows, cols, k)
    inp = Guarded(dev, flat, seed=1)
    marks_k = np.arange(rows * k, dtype=np.uint32) ^ np.uint32(0xa5a5a5a5)
    marks_i = np.arange(rows * k, dtype=np.uint32) ^ np.uint32(0x5a5a5a5a)
    ko = Guarded(dev, marks_k, guard_bytes=SENTINELS * 4, seed=2)
    io = Guarded(dev, marks_i, guard_bytes=SENTINELS * 4, seed=3)
    w = Guarded(dev, nbytes=wb, seed=4)
    sz = ctypes.c_size_t()
    call = lib.adlhip_topk_rows_typed

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    try:
        for algo in ALGOS:
            dev.setParam("topk.rows_algo", algo)
            h = dev._h
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, cols + 1, ko.ptr(), io.ptr(), w.ptr(), wb), "k > cols")
            refused(lib.adlhip_topk_rows_scratch_bytes(h, F32, rows, cols, cols + 1, ctypes.byref(sz)), "scratch, k > cols")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols - 1, k, ko.ptr(), io.ptr(), w.ptr(), wb), "row_stride < cols")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k, None, None, w.ptr(), wb), "both outputs null")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k - 1, ko.ptr(4), io.ptr(), w.ptr(), wb), "misaligned keys out")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k - 1, ko.ptr(), io.ptr(4), w.ptr(), wb), "misaligned index out")
            refused(call(h, F32, ASC, inp.ptr(4), rows, cols - 1, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb), "misaligned input")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(4), wb - 4), "misaligned work")
            assert str(wb) in refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb - 1),
                                      "work one byte short")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k, inp.ptr(16), io.ptr(), w.ptr(), wb), "keys out overlaps the input")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, k, ko.ptr(), inp.ptr(4 * (rows * cols - 4)), w.ptr(), wb),
                    "index out overlaps the last row")
            for bad in (-1, 6, 99):
                refused(call(h, bad, ASC, inp.ptr(), rows, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb), "key_type %d" % bad)
                refused(lib.adlhip_topk_rows_scratch_bytes(h, bad, rows, cols, k, ctypes.byref(sz)), "scratch, key_type %d" % bad)
            for bad in (-1, 2):
                refused(call(h, F32, bad, inp.ptr(), rows, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb), "order %d" % bad)
            # k == 0 and rows == 0 succeed and enqueue nothing
            assert call(h, F32, DESC, inp.ptr(), rows, cols, cols, 0, ko.ptr(), io.ptr(), w.ptr(), wb) == 0, lib_err()
            assert call(h, F32, DESC, inp.ptr(), 0, cols, cols, k, ko.ptr(), io.ptr(), w.ptr(), wb) == 0, lib_err()
            assert call(h, F32, DESC, None, 0, 0, 0, 0, None, None, None, 0) == 0, lib_err()
            assert np.array_equal(ko.read(np.uint32), marks_k) and np.array_equal(io.read(np.uint32), marks_i)
            assert np.array_equal(inp.read(np.uint32), flat)
            w.check_guard()
            assert dev.getParam("debug.idle_dirty") == 0
        assert rows_bytes(dev, F32, rows, cols, k) == wb
        one = ctypes.c_size_t()
        assert lib.adlhip_topk_scratch_bytes(dev._h, F32, cols, k, ctypes.byref(one)) == 0 and one.value == wb   # the 1-D call's size
    finally:
        dev.setParam("topk.rows_algo", -1)
        for b in (inp, ko, io, w):
            b.release()


# ---------------------------------------------------------------------------------------------
# the Python mirror
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    from oclradixsort_amd import Pprims
    rows, cols, stride, k = 6, 6007, 6010, 50
    bits = random_bits(np.uint64, (rows - 1) * stride + cols, seed=81)
    p = Pprims()
    keys = Buffer(dev, bits.size, np.float64)
    kout = Buffer(dev, rows * k, np.float64)
    try:
        keys.write(bits.view(np.float64))
        out = p.topkRows(dev, keys, rows, cols, k, descending=True, keysOut=kout, rowStride=stride)
        got = out.toHost().astype(np.int64).reshape(rows, k)
        got_k = kout.toHost().view(np.uint64).reshape(rows, k)
        for r in range(rows):
            row = bits[r * stride:r * stride + cols]
            want = expected_perm(row, "f64", DESC)[:k]
            assert np.array_equal(got[r], want) and np.array_equal(got_k[r], row[want])
        out.release()
        out = p.topkRows(dev, keys, rows, cols, 0)
        assert out.getSize() == 0
        out.release()
    finally:
        keys.release()
        kout.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# 11. torch parity
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(torch, dtype, shape):
    g = torch.Generator(device="cuda").manual_seed(11)
    if dtype.is_floating_point:
        t = torch.randn(shape, dtype=dtype, device="cuda", generator=g)
        return torch.where(t == 0, torch.ones_like(t), t)   # no -0 (and no +0 either), no NaN
    return torch.randint(-500, 500, shape, dtype=dtype, device="cuda", generator=g)   # many ties


@pytest.mark.parametrize("largest", [True, False], ids=["largest", "smallest"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_topk_rows_matches_torch(sorter, dtype_name, largest):
    import torch
    dtype = getattr(torch, dtype_name)
    for shape in ((37, 5001), (3, 5, 1000)):
        t = _torch_input(torch, dtype, shape)
        keep = t.clone()
        order = torch.sort(t, dim=-1, descending=largest, stable=True).indices
        for k in (1, 10, 300):
            values, indices = sorter.topk_rows(t, k, largest=largest)
            torch.cuda.synchronize()
            assert values.dtype == dtype and indices.dtype == torch.int64
            assert values.shape == shape[:-1] + (k,) and indices.shape == shape[:-1] + (k,)
            assert torch.equal(values, torch.topk(t, k, dim=-1, largest=largest, sorted=True).values)
            assert torch.equal(indices, order[..., :k])
        values, indices = sorter.topk_rows(t, 10, largest=largest, sorted=False)   # accepted; the output is sorted all the same
        assert torch.equal(indices, order[..., :10])
        values, indices = sorter.topk_rows(t, 0, largest=largest)
        assert values.shape == shape[:-1] + (0,) and indices.shape == shape[:-1] + (0,) and indices.dtype == torch.int64
        assert torch.equal(t, keep), "the input was changed"
        with pytest.raises(ValueError):
            sorter.topk_rows(t, shape[-1] + 1)
        with pytest.raises(ValueError):
            sorter.topk_rows(t, -1)
    base = _torch_input(torch, dtype, (5001, 37))
    tt = base.t()   # 37 x 5001, transposed
    assert not tt.is_contiguous()
    keep = base.clone()
    values, indices = sorter.topk_rows(tt, 20, largest=largest)
    assert torch.equal(values, torch.topk(tt, 20, dim=-1, largest=largest).values)
    assert torch.equal(indices, torch.sort(tt, dim=-1, descending=largest, stable=True).indices[..., :20])
    assert torch.equal(base, keep), "the input was changed"
    # contiguous views that start at an odd offset (the ABI wants the base pointer on 16 bytes), and a view strided by columns
    m = _torch_input(torch, dtype, (65, 33))
    keep = m.clone()
    assert m[1:].is_contiguous() and m[1:].data_ptr() % 16 and not m[:, 1:].is_contiguous()
    for view in (m[1:], m[3:], m[:, 1:], m[1:, 1:]):
        order = torch.sort(view, dim=-1, descending=largest, stable=True).indices
        for k in (1, 7, view.shape[-1]):
            values, indices = sorter.topk_rows(view, k, largest=largest)
            assert values.shape == (view.shape[0], k) and indices.shape == (view.shape[0], k)
            assert torch.equal(values, torch.topk(view, k, dim=-1, largest=largest, sorted=True).values)
            assert torch.equal(indices, order[..., :k])
    values, indices = sorter.topk_rows(m[1:1], 5, largest=largest)   # no rows, at an odd offset
    assert values.shape == (0, 5) and indices.shape == (0, 5) and indices.dtype == torch.int64
    assert torch.equal(m, keep), "the input was changed"


def test_torch_sorter_topk_rows_refusals(sorter, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.arange(200, dtype=torch.int32, device="cuda").reshape(2, 100)
    monkeypatch.setattr(sorter.pprims, "topkRows", boom)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        with pytest.raises(RuntimeError):
            sorter.topk_rows(t, 3)
    with pytest.raises(ValueError):
        sorter.topk_rows(torch.arange(100, dtype=torch.int32, device="cuda"), 3)       # 1-D: topk serves it
    with pytest.raises(TypeError):
        sorter.topk_rows(torch.zeros((4, 4), dtype=torch.float16, device="cuda"), 1)
    with pytest.raises(ValueError):
        sorter.topk_rows(torch.zeros((4, 4), dtype=torch.float32), 1)                  # a CPU tensor
    with pytest.raises(TypeError):
        sorter.topk_rows([[3.0, 1.0]], 1)
    monkeypatch.undo()
    values, indices = sorter.topk_rows(t, 3)
    assert values.tolist() == [[99, 98, 97], [199, 198, 197]] and indices.tolist() == [[99, 98, 97]] * 2
    with pytest.raises(ValueError):
        sorter.topk(torch.zeros((4, 4), dtype=torch.float32, device="cuda"), 1)        # topk keeps refusing 2-D input
    values, indices = sorter.topk(t[1], 2)
    assert values.tolist() == [199, 198] and indices.tolist() == [99, 98]
