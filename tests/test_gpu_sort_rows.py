"""Sort and argsort along rows on the GPU (include/adlhip.h adlhip_sort_rows_typed; oclradixsort_amd/csrc/sortrows_kernels.hpp;
Pprims.sortRows; TorchSorter.sort_rows / argsort_rows).

The expected output is independent of the code under test: the keys are encoded with the numpy codec of tests/typed_shapes.py
(encoded_dwords: a key's ordinal moved into the unsigned range; descending: its complement) and every row's expectation is
np.argsort(codes_row, kind="stable").  Indices and key bits must be equal; there is no tolerance anywhere.

Every call of run() checks the whole memory contract: both outputs lie between canary regions that are unchanged afterwards, the
input -- the gap elements between cols and row_stride and the canaries around it included -- is unchanged, the work buffer has exactly
the reported size, holds garbage on entry and has canaries of its own (the row kernel reports 0 bytes and must leave all of it alone),
adlhip_fault_check is clean and "debug.idle_dirty" reads 0.  Calls of different shapes follow each other on one handle throughout.

The ABI wants the BASE pointer of the input on 16 bytes and refuses any other, so no view can start at an odd element.  The input
view here starts 48 bytes (an odd multiple of 16) into a larger allocation, and the spans the row kernel loads start at odd elements
wherever rows-per-tile * cols * key bytes is no multiple of 16 (cols odd with one or two rows per tile), as strided rows do.

G below is the number of rows a tile of the row kernel takes: 4096 / P, P the power of two >= cols, at least 2.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, _lib
from typed_shapes import ASC, BY_NAME, DESC, SPECIALS, encoded_dwords

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "sort_rows_demo")
TYPE_IDS = ["u32", "i32", "f32", "u64", "i64", "f64"]
CAP = 4096
KERNEL, FLAT, AUTO = 1, 0, -1
BOTH, KEYS_ONLY, INDEX_ONLY = "both", "keys", "index"
MODES = (BOTH, KEYS_ONLY, INDEX_ONLY)
MAX_ELEMS = 64 << 10   # rows * cols of a row-kernel case at most


def rows_per_tile(cols):
    p = 2
    while p < cols:
        p *= 2
    return CAP // p


# ---------------------------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------------------------
def codes_of(bits, name, order):
    """the unsigned codes whose ascending order is the requested order of the keys (typed_shapes' codec; 8-byte keys as one uint64)"""
    low, high = encoded_dwords(bits, name)
    code = low.astype(np.uint64) if high is None else (high.astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    if order == DESC:
        code = ~code if high is not None else (~code) & np.uint64(0xffffffff)
    return code


def expected_rows(flat, name, rows, cols, stride, order):
    """(columns [rows, cols] int64, key bits [rows, cols]) of the stable argsort of every row"""
    at = (np.arange(rows, dtype=np.int64) * stride)[:, None] + np.arange(cols, dtype=np.int64)[None, :]
    m = flat[at]
    codes = codes_of(m.reshape(-1), name, order).reshape(rows, cols)
    perm = np.argsort(codes, axis=1, kind="stable")
    return perm.astype(np.int64), np.take_along_axis(m, perm, axis=1)


def random_bits(udt, n, seed, specials=True):
    rng = np.random.default_rng(seed)
    w = np.dtype(udt).itemsize
    x = np.frombuffer(rng.bytes(w * max(n, 1)), dtype=udt)[:n].copy()
    if specials and n >= 8:   # +-NaN of several payloads, +-0, +-inf, denormals, the extremes of the integer readings
        sp = SPECIALS[w]
        at = rng.choice(n, size=min(n // 2, 3 * sp.size), replace=False)
        x[at] = np.resize(sp, at.size)
    return x


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
def lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


def reset(d):
    d.setParam("sort.rows_algo", -1)
    d.setParam("debug.sort_rows_grid", 0)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    reset(d)
    DeviceUtils.deallocate(d)


class Framed:
    """nbytes of payload on the device between two canary regions; the payload starts `front` bytes (a multiple of 16) into the
    allocation.  `payload`: its bytes; otherwise it is filled with `fill`."""

    def __init__(self, dev, nbytes=None, payload=None, front=256, back=256, fill=0xcd, seed=1):
        rng = np.random.default_rng(seed)
        if payload is not None:
            body = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
        else:
            body = np.full(int(nbytes), fill, np.uint8)
        self.dev, self.front, self.nbytes = dev, front, body.size
        self.image = np.concatenate([rng.integers(0, 256, size=front, dtype=np.uint8), body,
                                     rng.integers(0, 256, size=back, dtype=np.uint8)])
        self.buf = Buffer(dev, self.image.size, np.uint8)
        self.buf.write(self.image)

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.buf.m_ptr + self.front + offset)

    def read(self, dtype=np.uint8):
        """the payload; asserts that the canaries are what they were"""
        raw = self.buf.toHost()
        a, b = self.front, self.front + self.nbytes
        assert np.array_equal(raw[:a], self.image[:a]), "bytes in front of the buffer were written"
        assert np.array_equal(raw[b:], self.image[b:]), "bytes behind the buffer were written"
        return raw[a:b].view(dtype)

    def unchanged(self):
        return np.array_equal(self.read(), self.image[self.front:self.front + self.nbytes])

    def release(self):
        self.buf.release()


def scratch_bytes(dev, kt, rows, cols):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_sort_rows_scratch_bytes(dev._h, kt, rows, cols, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Case:
    """rows x cols keys at a row stride on the device and every order's expectation (computed once)"""

    def __init__(self, dev, name, flat, rows, cols, stride=None):
        self.dev, self.name, self.kt, self.udt = dev, name, BY_NAME[name][1], BY_NAME[name][3]
        self.rows, self.cols, self.stride = rows, cols, cols if stride is None else stride
        assert flat.dtype == self.udt and flat.size == (rows - 1) * self.stride + cols
        self.flat = flat
        self.inp = Framed(dev, payload=flat, front=48, seed=5)   # 48: the view starts at an odd multiple of 16 bytes
        self._want = {}

    def expected(self, order):
        if order not in self._want:
            self._want[order] = expected_rows(self.flat, self.name, self.rows, self.cols, self.stride, order)
        return self._want[order]

    def run(self, order, mode=BOTH):
        """one call under the knobs in force; returns (index bytes or None, key bytes or None) after every check"""
        w_item = self.flat.dtype.itemsize
        n = self.rows * self.cols
        need = scratch_bytes(self.dev, self.kt, self.rows, self.cols)
        ko = Framed(self.dev, nbytes=n * w_item, seed=6) if mode != INDEX_ONLY else None
        io = Framed(self.dev, nbytes=n * 4, seed=7) if mode != KEYS_ONLY else None
        work = Framed(self.dev, nbytes=max(need, 16), fill=0xa7, seed=8)   # garbage on entry
        try:
            rc = _lib.load().adlhip_sort_rows_typed(self.dev._h, self.kt, order, self.inp.ptr(), self.rows, self.cols, self.stride,
                                                    ko.ptr() if ko else None, io.ptr() if io else None, work.ptr(), need)
            assert rc == 0, lib_err()
            got_i = io.read(np.uint32).reshape(self.rows, self.cols) if io else None
            got_k = ko.read(self.udt).reshape(self.rows, self.cols) if ko else None
            after = work.read()   # (checks the canaries of the work buffer)
            if need == 0:
                assert (after == 0xa7).all(), "the row kernel wrote to d_work"
            assert self.inp.unchanged(), "the sort changed d_keys_in (or the gaps between its rows)"
            self.dev.checkFault()
            assert self.dev.getParam("debug.idle_dirty") == 0
            want_i, want_k = self.expected(order)
            what = "%s order %d rows %d cols %d stride %d %s" % (self.name, order, self.rows, self.cols, self.stride, mode)
            if io:
                bad = np.flatnonzero((got_i.astype(np.int64) != want_i).any(axis=1))
                assert bad.size == 0, "%s: columns differ in rows %s" % (what, bad[:8].tolist())
            if ko:
                bad = np.flatnonzero((got_k != want_k).any(axis=1))
                assert bad.size == 0, "%s: keys differ in rows %s" % (what, bad[:8].tolist())
            return (got_i.tobytes() if io else None, got_k.tobytes() if ko else None)
        finally:
            for b in (ko, io, work):
                if b is not None:
                    b.release()

    def run_both_paths(self, order, mode=BOTH):
        """the row kernel and the flat path on the same input: each against numpy, and identical bytes"""
        try:
            self.dev.setParam("sort.rows_algo", KERNEL)
            a = self.run(order, mode)
            self.dev.setParam("sort.rows_algo", FLAT)
            b = self.run(order, mode)
        finally:
            self.dev.setParam("sort.rows_algo", AUTO)
        assert a == b, "the two paths disagree"

    def release(self):
        self.inp.release()


def make_case(dev, name, rows, cols, stride=None, seed=0, bits=None):
    stride = cols if stride is None else stride
    n = (rows - 1) * stride + cols
    flat = random_bits(BY_NAME[name][3], n, seed) if bits is None else bits(n)
    return Case(dev, name, np.ascontiguousarray(flat, dtype=BY_NAME[name][3]), rows, cols, stride)


# ---------------------------------------------------------------------------------------------
# 1. the row kernel: edge sizes, strides, output modes
# ---------------------------------------------------------------------------------------------
EDGE_COLS = [1, 2, 3, 31, 32, 33, 255, 256, 257, 2048, 2049, 4095, 4096]


def edge_rows(cols):
    g = rows_per_tile(cols)
    return sorted(set(r for r in (1, 2, 3, g - 1, g, g + 1, 3 * g + 1) if 1 <= r and r * cols <= MAX_ELEMS))


@pytest.mark.parametrize("cols", EDGE_COLS)
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_row_kernel_edge_sizes(dev, name, cols):
    """rows around a tile's G, strides cols, cols + 1 and cols + 7, both orders; keys only, indices only and both in turn"""
    dev.setParam("sort.rows_algo", KERNEL)
    turn = 0
    try:
        for rows in edge_rows(cols):
            for stride in (cols, cols + 1, cols + 7):
                c = make_case(dev, name, rows, cols, stride, seed=1000 * cols + 10 * rows + stride)
                try:
                    for order in (ASC, DESC):
                        c.run(order, MODES[turn % 3])
                        turn += 1
                finally:
                    c.release()
        assert turn >= 3
    finally:
        dev.setParam("sort.rows_algo", AUTO)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_few_workgroups_walk_many_tiles(dev, name, grid):
    """3 G + 1 rows: four tiles, the last one with a single row, taken by one and by three workgroups"""
    dev.setParam("sort.rows_algo", KERNEL)
    dev.setParam("debug.sort_rows_grid", grid)
    try:
        assert dev.getParam("debug.sort_rows_grid") == grid
        for cols in (3, 33, 257, 2049, 4095):
            rows = 3 * rows_per_tile(cols) + 1
            assert rows * cols <= MAX_ELEMS
            for stride in (cols, cols + 1):
                c = make_case(dev, name, rows, cols, stride, seed=77 * cols + stride)
                try:
                    c.run(ASC if cols % 2 else DESC)
                finally:
                    c.release()
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 2. every type and order with the special bit patterns; both paths, the same bytes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_every_type_and_order_on_both_paths(dev, name, order):
    w = np.dtype(BY_NAME[name][3]).itemsize
    for cols, stride in ((33, 33), (257, 264), (4096, 4096)):
        rows = min(rows_per_tile(cols) + 1, MAX_ELEMS // cols)
        c = make_case(dev, name, rows, cols, stride, seed=31 * cols + w)
        try:
            assert np.isin(SPECIALS[w], c.flat).all()
            c.run_both_paths(order)
        finally:
            c.release()


# ---------------------------------------------------------------------------------------------
# 3. ties: keys drawn from {0, 1}, and all keys equal -- the columns decide, ascending in both orders
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "u64"])
def test_ties_are_broken_by_ascending_column(dev, name):
    udt = BY_NAME[name][3]
    for cols, stride in ((5, 5), (33, 34), (300, 300), (4096, 4103)):
        rows = min(2 * rows_per_tile(cols) + 1, 8192 // cols + 1)
        two = make_case(dev, name, rows, cols, stride, bits=lambda n: np.random.default_rng(cols).integers(0, 2, size=n).astype(udt))
        same = make_case(dev, name, rows, cols, stride, bits=lambda n: np.full(n, 0x3f800000, dtype=udt))
        try:
            for order in (ASC, DESC):
                two.run_both_paths(order)
                same.run_both_paths(order)
                assert np.array_equal(same.expected(order)[0], np.tile(np.arange(cols), (rows, 1)))
        finally:
            two.release()
            same.release()


# ---------------------------------------------------------------------------------------------
# 4. the flat path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 5), (2, 3), (7, 5), (16, 9), (17, 9), (257, 3)])
def test_flat_path_at_tiny_shapes(dev, rows, cols):
    """the bit length of rows - 1 goes through 0, 1, 3, 4, 5 and 9: sort_bits of the (row, position) sort is 4, 8 and 12"""
    dev.setParam("sort.rows_algo", FLAT)
    turn = 0
    try:
        for name in ("f32", "i64"):
            for stride in (cols, cols + 3):
                c = make_case(dev, name, rows, cols, stride, seed=rows * 100 + cols + stride)
                ties = make_case(dev, name, rows, cols, stride,
                                 bits=lambda n: np.random.default_rng(rows).integers(0, 2, size=n).astype(BY_NAME[name][3]))
                try:
                    for order in (ASC, DESC):
                        c.run(order, MODES[turn % 3])
                        ties.run(order, MODES[(turn + 1) % 3])
                        turn += 1
                finally:
                    c.release()
                    ties.release()
    finally:
        dev.setParam("sort.rows_algo", AUTO)


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_flat_path_by_default_above_4096_columns(dev, name):
    assert dev.getParam("sort.rows_algo") == AUTO
    for rows in (1, 3):
        for stride in (4097, 4100):
            c = make_case(dev, name, rows, 4097, stride, seed=4097 + rows + stride)
            try:
                assert scratch_bytes(dev, c.kt, rows, 4097) > 0   # (the row kernel would report 0)
                for order in (ASC, DESC):
                    c.run(order)
            finally:
                c.release()


@pytest.mark.parametrize("name,order", [("f32", DESC), ("u64", ASC)])
def test_flat_path_where_the_argsort_leaves_its_small_sort(dev, name, order):
    udt = BY_NAME[name][3]
    c = make_case(dev, name, 5, 70001, seed=70001)
    ties = make_case(dev, name, 5, 70001, 70004, bits=lambda n: np.random.default_rng(3).integers(0, 37, size=n).astype(udt))
    try:
        c.run(order)
        ties.run(order, INDEX_ONLY)
    finally:
        c.release()
        ties.release()


# ---------------------------------------------------------------------------------------------
# 5. refusals: each by its message, and nothing written
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32 = 2
    call = lib.adlhip_sort_rows_typed
    sz = ctypes.c_size_t()
    for algo, rows, cols in ((KERNEL, 40, 100), (FLAT, 40, 100), (AUTO, 3, 5000)):
        dev.setParam("sort.rows_algo", algo)
        n = rows * cols
        flat = random_bits(np.uint32, n, seed=71)
        wb = scratch_bytes(dev, F32, rows, cols)
        assert (wb == 0) == (algo == KERNEL)
        inp = Framed(dev, payload=flat, seed=1)
        ko = Framed(dev, payload=np.arange(n, dtype=np.uint32) ^ np.uint32(0xa5a5a5a5), seed=2)
        io = Framed(dev, payload=np.arange(n, dtype=np.uint32) ^ np.uint32(0x5a5a5a5a), seed=3)
        w = Framed(dev, nbytes=max(wb, 64), fill=0xa7, seed=4)
        h = dev._h

        def refused(rc, *words):
            assert rc == 1, words
            msg = lib_err()
            for word in words:
                assert word in msg, (words, msg)

        try:
            refused(call(h, F32, ASC, None, rows, cols, cols, ko.ptr(), io.ptr(), w.ptr(), wb), "d_keys_in", "NULL")
            refused(call(h, F32, ASC, inp.ptr(4), rows, cols - 1, cols, ko.ptr(), io.ptr(), w.ptr(), wb), "d_keys_in", "16-byte")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(4), io.ptr(), w.ptr(), wb), "d_keys_out", "16-byte")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(8), w.ptr(), wb), "d_index_out", "16-byte")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(), w.ptr(4), wb), "d_work", "16-byte")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, None, None, w.ptr(), wb), "d_keys_out", "d_index_out")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, inp.ptr(16), io.ptr(), w.ptr(), wb), "d_keys_out", "overlap")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), inp.ptr(4 * (n - 4)), w.ptr(), wb), "d_index_out", "overlap")
            refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols - 1, ko.ptr(), io.ptr(), w.ptr(), wb), "row_stride")
            for bad in (-1, 6, 99):
                refused(call(h, bad, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(), w.ptr(), wb), "key_type")
                refused(lib.adlhip_sort_rows_scratch_bytes(h, bad, rows, cols, ctypes.byref(sz)), "key_type")
            for bad in (-1, 2):
                refused(call(h, F32, bad, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(), w.ptr(), wb), "order")
            refused(call(h, F32, ASC, inp.ptr(), 1 << 20, 1 << 12, 1 << 12, ko.ptr(), io.ptr(), w.ptr(), wb), "rows * cols")
            refused(lib.adlhip_sort_rows_scratch_bytes(h, F32, 1 << 20, 1 << 12, ctypes.byref(sz)), "rows * cols")
            refused(call(h, F32, ASC, inp.ptr(), 1 << 40, 1 << 40, 1 << 40, ko.ptr(), io.ptr(), w.ptr(), wb), "rows * cols")
            if wb:
                refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(), w.ptr(), wb - 1), "work_bytes", str(wb))
                refused(call(h, F32, ASC, inp.ptr(), rows, cols, cols, ko.ptr(), io.ptr(), None, wb), "d_work", "NULL")
            # rows == 0 and cols == 0 succeed and enqueue nothing
            assert call(h, F32, DESC, inp.ptr(), 0, cols, cols, ko.ptr(), io.ptr(), w.ptr(), wb) == 0, lib_err()
            assert call(h, F32, DESC, inp.ptr(), rows, 0, cols, ko.ptr(), io.ptr(), w.ptr(), wb) == 0, lib_err()
            assert call(h, F32, DESC, None, 0, 0, 0, None, None, None, 0) == 0, lib_err()
            assert lib.adlhip_sort_rows_scratch_bytes(h, F32, 0, cols, ctypes.byref(sz)) == 0 and sz.value == 0
            assert ko.unchanged() and io.unchanged() and inp.unchanged() and w.unchanged(), "a refused call wrote something"
            dev.checkFault()
            assert dev.getParam("debug.idle_dirty") == 0
        finally:
            dev.setParam("sort.rows_algo", AUTO)
            for b in (inp, ko, io, w):
                b.release()


def test_the_row_kernel_refuses_more_than_4096_columns(dev):
    lib = _lib.load()
    F32, rows, cols = 2, 2, 4097
    sz = ctypes.c_size_t()
    inp = Framed(dev, payload=random_bits(np.uint32, rows * cols, seed=9))
    io = Framed(dev, nbytes=4 * rows * cols)
    w = Framed(dev, nbytes=64)
    try:
        dev.setParam("sort.rows_algo", KERNEL)
        assert lib.adlhip_sort_rows_typed(dev._h, F32, ASC, inp.ptr(), rows, cols, cols, None, io.ptr(), w.ptr(), 64) == 1
        assert "sort.rows_algo" in lib_err() and "4096" in lib_err(), lib_err()
        assert lib.adlhip_sort_rows_scratch_bytes(dev._h, F32, rows, cols, ctypes.byref(sz)) == 1
        assert "sort.rows_algo" in lib_err() and "4096" in lib_err(), lib_err()
        assert io.unchanged() and inp.unchanged() and w.unchanged()
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        dev.setParam("sort.rows_algo", AUTO)
        for b in (inp, io, w):
            b.release()


# ---------------------------------------------------------------------------------------------
# 6. the knobs
# ---------------------------------------------------------------------------------------------
def test_knobs_round_trip_and_leave_the_others_alone(dev):
    others = ["topk.rows_algo", "debug.topk_rows_grid", "topk.algo", "sort.algo", "sort.mid", "unique.algo", "debug.unique_grid",
              "debug.search_grid", "sort.digit_bits"]
    before = [dev.getParam(k) for k in others]
    try:
        assert dev.getParam("sort.rows_algo") == -1 and dev.getParam("debug.sort_rows_grid") == 0
        for v in (0, 1, -1):
            dev.setParam("sort.rows_algo", v)
            assert dev.getParam("sort.rows_algo") == v
        for v in (1, 3, 100000, 0):
            dev.setParam("debug.sort_rows_grid", v)
            assert dev.getParam("debug.sort_rows_grid") == v
        for bad in (-2, 2, 17):
            with pytest.raises(Exception, match="sort.rows_algo"):
                dev.setParam("sort.rows_algo", bad)
        with pytest.raises(Exception, match="debug.sort_rows_grid"):
            dev.setParam("debug.sort_rows_grid", -1)
        assert dev.getParam("sort.rows_algo") == -1 and dev.getParam("debug.sort_rows_grid") == 0
        assert [dev.getParam(k) for k in others] == before
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 7. the Python mirror, torch, the facade
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    from oclradixsort_amd import Pprims
    p = Pprims()
    try:
        for rows, cols, stride in ((6, 607, 610), (2, 6007, 6007)):   # the row kernel (no scratch at all), the flat path
            bits = random_bits(np.uint64, (rows - 1) * stride + cols, seed=81 + cols)
            keys = Buffer(dev, bits.size, np.float64)
            kout = Buffer(dev, rows * cols, np.float64)
            try:
                keys.write(bits.view(np.float64))
                out = p.sortRows(dev, keys, rows, cols, descending=True, keysOut=kout, rowStride=stride)
                got = out.toHost().astype(np.int64).reshape(rows, cols)
                got_k = kout.toHost().view(np.uint64).reshape(rows, cols)
                out.release()
                want_i, want_k = expected_rows(bits, "f64", rows, cols, stride, DESC)
                assert np.array_equal(got, want_i) and np.array_equal(got_k, want_k)
                out = p.sortRows(dev, keys, 0, cols)
                assert out.getSize() == 0
                out.release()
            finally:
                keys.release()
                kout.release()
    finally:
        p.close()


@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(dtype, shape):
    g = torch.Generator(device="cuda").manual_seed(11)
    if dtype.is_floating_point:
        t = torch.randn(shape, dtype=dtype, device="cuda", generator=g)
        return torch.where(t == 0, torch.ones_like(t), t)   # no -0 (and no +0 either), no NaN
    return torch.randint(-50, 50, shape, dtype=dtype, device="cuda", generator=g)   # many ties


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_sort_rows_matches_torch(sorter, dtype_name, descending):
    dtype = getattr(torch, dtype_name)
    inputs = [_torch_input(dtype, shape) for shape in ((3, 5), (2, 3, 33), (4, 4097), (0, 5), (3, 0))]
    odd = _torch_input(dtype, (6, 33))[1:]   # contiguous, but it starts at an odd offset
    assert odd.is_contiguous() and odd.data_ptr() % 16
    for t in inputs + [odd]:
        keep = t.clone()
        want = torch.sort(t.cpu(), dim=-1, descending=descending, stable=True)
        values, indices = sorter.sort_rows(t, descending=descending)
        only = sorter.argsort_rows(t, descending=descending)
        torch.cuda.synchronize()
        assert values.dtype == dtype and indices.dtype == torch.int64 and only.dtype == torch.int64
        assert values.shape == t.shape and indices.shape == t.shape and only.shape == t.shape
        assert torch.equal(values.cpu(), want.values)
        assert torch.equal(indices.cpu(), want.indices) and torch.equal(only.cpu(), want.indices)
        assert torch.equal(t, keep), "the input was changed"


def test_torch_sorter_sort_rows_refusals(sorter, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.arange(200, dtype=torch.int32, device="cuda").reshape(2, 100)
    monkeypatch.setattr(sorter.pprims, "sortRows", boom)
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(RuntimeError):
            sorter.sort_rows(t)
    with pytest.raises(ValueError):
        sorter.sort_rows(torch.arange(100, dtype=torch.int32, device="cuda"))        # 1-D: sort serves it
    with pytest.raises(TypeError):
        sorter.argsort_rows(torch.zeros((4, 4), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        sorter.sort_rows(torch.zeros((4, 4), dtype=torch.float32))                   # a CPU tensor
    with pytest.raises(TypeError):
        sorter.sort_rows([[3.0, 1.0]])
    monkeypatch.undo()
    values, indices = sorter.sort_rows(t, descending=True)
    assert values[:, :3].tolist() == [[99, 98, 97], [199, 198, 197]] and indices[:, :3].tolist() == [[99, 98, 97]] * 2
    with pytest.raises(ValueError):
        sorter.sort(torch.zeros((4, 4), dtype=torch.float32, device="cuda"))          # sort keeps refusing 2-D input


def test_sort_rows_demo_on_the_device_prints_what_the_host_path_prints():
    def lines(args):
        r = subprocess.run([DEMO, "--dump"] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.startswith("[") or ln.startswith("DUMP ")]

    device, host = lines([]), lines(["--host"])
    assert len(device) == 12 * 7 + 12 * 4 and all(ln.startswith("[ OK ] SortRows.") for ln in device if ln.startswith("["))
    assert device == host
