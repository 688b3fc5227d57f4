"""Histograms on the GPU (include/adlhip.h "histograms"; oclradixsort_amd/csrc/histogram_kernels.hpp; Pprims.histogramRange / binCount;
TorchSorter.bincount / histogram / histc).

The oracle is tests/histogram_oracle.py (numpy on key codes; tests/test_histogram_api.py checks it against a plain loop and against
numpy.histogram on the CPU).  Every case is compared bit for bit.

Every call runs on guarded device buffers: keys, edges, the counters (sized exactly num_bins, prefilled with sentinels) and a work buffer
of exactly the reported bytes carry guard bytes behind their payload, and the inputs are compared with their originals afterwards.  The
handle's device state is idle after each case.  T is the tile of the count kernel, read from the binding, which a CPU test compares
with the header's ADLHIP_HISTOGRAM_TILE."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from histogram_oracle import BY_NAME, INT_IDS, SPECIAL_KEYS, TYPE_IDS, bincount_oracle, encode, histogram_range_oracle, sort_edges
from oclradixsort_amd import DeviceUtils, _lib
from oclradixsort_amd.pprims import HISTOGRAM_MAX_RANGE_BINS, HISTOGRAM_TILE
from test_gpu_reduce import Guarded, lib_err, sentinels
from test_histogram_api import DEMO, check_demo_output

pytestmark = pytest.mark.gpu

T = HISTOGRAM_TILE
SIZES = [0, 1, 3, T - 1, T, T + 1, 5 * T + 7]
GRIDS = [0, 1, 2, 7, 64]
SENTINELS = 64


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.histogram_grid", 0)
    d.setParam("debug.histogram_lds_bins", 0)
    DeviceUtils.deallocate(d)


@pytest.fixture(scope="module")
def lds_limit(dev):
    return dev.getParam("debug.histogram_lds_bins")


def scratch_bytes(dev, name, n, bins, by_edges):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_histogram_scratch_bytes(dev._h, BY_NAME[name][1], n, bins, by_edges, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def random_bits(udt, n, rng):
    w = np.dtype(udt).itemsize
    return np.frombuffer(rng.bytes(w * max(n, 1)), dtype=udt)[:n].copy()


class Case:
    """guarded keys (and edges), sentinel-filled counters sized exactly num_bins, a work buffer of exactly the reported bytes"""

    def __init__(self, dev, name, kbits, ebits, bins, fill=None):
        self.dev, self.name, self.kbits, self.ebits, self.bins = dev, name, kbits, ebits, bins
        self.keys = Guarded(dev, kbits, guard_bytes=SENTINELS * kbits.dtype.itemsize, seed=5)
        self.edges = Guarded(dev, ebits, guard_bytes=SENTINELS * ebits.dtype.itemsize, seed=6) if ebits is not None else None
        self.sent = sentinels(np.uint32, bins, 0xa5a5a5a5a5a5a5a5)
        self.counts = Guarded(dev, self.sent, guard_bytes=SENTINELS * 4, seed=20)
        self.work = Guarded(dev, nbytes=scratch_bytes(dev, name, kbits.size, bins, 1 if ebits is not None else 0), seed=8, fill=fill)

    def reset(self):
        self.counts.buf.write(self.sent.view(np.uint8))

    def call(self, include_upper=0, work_bytes=None, n=None):
        lib = _lib.load()
        wb = self.work.nbytes if work_bytes is None else work_bytes
        n = self.kbits.size if n is None else n
        if self.ebits is not None:
            return lib.adlhip_histogram_range_typed(self.dev._h, BY_NAME[self.name][1], self.keys.ptr(), n, self.edges.ptr(), self.bins,
                                                    include_upper, self.counts.ptr(), self.work.ptr(), wb)
        return lib.adlhip_bincount_typed(self.dev._h, BY_NAME[self.name][1], self.keys.ptr(), n, self.bins, self.counts.ptr(), self.work.ptr(), wb)

    def check(self, want, what):
        got = self.counts.read(np.uint32)   # (checks the guard behind the counters)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%s: counts differ in %d of %d bins, first in bin %d: got %d, expected %d"
                                 % (what, bad.size, want.size, bad[0], int(got[bad[0]]), int(want[bad[0]])))
        self.inputs_intact(what)
        assert self.dev.getParam("debug.idle_dirty") == 0
        return got

    def inputs_intact(self, what=""):
        self.work.check_guard()
        assert np.array_equal(self.keys.read(self.kbits.dtype), self.kbits), "%s: the keys were changed" % what
        if self.edges is not None:
            assert np.array_equal(self.edges.read(self.ebits.dtype), self.ebits), "%s: the edges were changed" % what

    def untouched(self):
        assert np.array_equal(self.counts.read(np.uint32), self.sent), "the counters were written"
        self.inputs_intact()

    def release(self):
        for b in (self.keys, self.edges, self.counts, self.work):
            if b is not None:
                b.release()


def run_range(dev, name, kbits, ebits, uppers=(0, 1), grid=0, fill=None):
    c = Case(dev, name, kbits, ebits, ebits.size - 1, fill=fill)
    dev.setParam("debug.histogram_grid", grid)
    res = {}
    try:
        for upper in uppers:
            c.reset()
            what = "range %s bins %d n %d grid %d upper %d" % (name, ebits.size - 1, kbits.size, grid, upper)
            assert c.call(upper) == 0, what + ": " + lib_err()
            res[upper] = c.check(histogram_range_oracle(kbits, name, ebits, bool(upper)), what)
    finally:
        dev.setParam("debug.histogram_grid", 0)
        c.release()
    return res


def run_bincount(dev, name, kbits, bins, grid=0, lds_bins=0, fill=None):
    dev.setParam("debug.histogram_lds_bins", lds_bins)   # before the work buffer is sized
    dev.setParam("debug.histogram_grid", grid)
    c = None
    try:
        c = Case(dev, name, kbits, None, bins, fill=fill)
        what = "bincount %s bins %d n %d grid %d lds_bins %d" % (name, bins, kbits.size, grid, lds_bins)
        assert c.call() == 0, what + ": " + lib_err()
        return c.check(bincount_oracle(kbits, name, bins), what)
    finally:
        dev.setParam("debug.histogram_grid", 0)
        dev.setParam("debug.histogram_lds_bins", 0)
        if c is not None:
            c.release()


def edges_of(name, bins, rng, kind="distinct"):
    """bins + 1 sorted edges of random bits; "repeated": every third copies its neighbour; "all_equal" """
    e = random_bits(BY_NAME[name][3], bins + 1, rng)
    if kind == "repeated":
        e[1::3] = e[0:-1:3][:e[1::3].size]
    if kind == "all_equal":
        e[:] = e[0]
    return sort_edges(e, name)


def keys_for(name, n, edges, rng):
    """random bits -- below, inside and above the edges --, every third key equal to an edge (the first and the last among them)"""
    k = random_bits(BY_NAME[name][3], n, rng)
    if n:
        pick = rng.integers(0, edges.size, size=k[::3].size)
        pick[:2] = (0, edges.size - 1)[:pick[:2].size]
        k[::3] = edges[pick]
    return k


def int_keys(name, n, bins, rng):
    """integers of which about half lie in [0, bins): negatives, bins itself, values far above, for 8-byte keys above 2^32"""
    sdt, udt = BY_NAME[name][2], BY_NAME[name][3]
    v = rng.integers(-(bins // 2) - 2, 2 * bins + 2, size=n).astype(np.int64)
    if n >= 8:
        v[1], v[2], v[3] = bins, bins - 1, 0
        v[4::16] = rng.integers(-(1 << 31), 1 << 31, size=v[4::16].size) if udt == np.uint32 else \
            rng.integers(-(1 << 62), 1 << 62, size=v[4::16].size)
        if udt == np.uint64:
            v[5::16] = (1 << 32) + rng.integers(0, bins, size=v[5::16].size)   # the low dword alone would be in range
    return v.astype(sdt).view(udt)   # (negative values of an unsigned type wrap to large ones)


# ---------------------------------------------------------------------------------------------
# sizes x grids
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_grids(dev, n, grid):
    rng = np.random.default_rng(1000 + n + grid)
    e = edges_of("f32", 65, rng)
    run_range(dev, "f32", keys_for("f32", n, e, rng), e, grid=grid)
    e = edges_of("i64", 64, rng, "repeated")
    run_range(dev, "i64", keys_for("i64", n, e, rng), e, grid=grid)
    run_bincount(dev, "i32", int_keys("i32", n, 1000, rng), 1000, grid=grid)
    run_bincount(dev, "u64", int_keys("u64", n, 3, rng), 3, grid=grid)


# ---------------------------------------------------------------------------------------------
# range mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 2, 63, 64, 65, 256, HISTOGRAM_MAX_RANGE_BINS - 1, HISTOGRAM_MAX_RANGE_BINS])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_range_every_type_and_bin_count(dev, name, bins):
    rng = np.random.default_rng(7 * bins + BY_NAME[name][1])
    n = T + 531
    for kind in ("distinct", "repeated", "all_equal"):
        e = edges_of(name, bins, rng, kind)
        run_range(dev, name, keys_for(name, n, e, rng), e, grid=3 if kind == "repeated" else 0)


@pytest.mark.parametrize("name", TYPE_IDS)
def test_range_every_key_on_an_edge(dev, name):
    rng = np.random.default_rng(3)
    for kind in ("distinct", "repeated"):
        e = edges_of(name, 100, rng, kind)
        k = e[rng.integers(0, e.size, size=T + 9)]
        res = run_range(dev, name, k, e)
        assert int(res[1].sum()) == k.size and int(res[0].sum()) == k.size - np.count_nonzero(k == e[-1])


@pytest.mark.parametrize("name", TYPE_IDS)
def test_range_special_keys_as_keys_and_as_edges(dev, name):
    rng = np.random.default_rng(4)
    sp = SPECIAL_KEYS[name]
    e = sort_edges(sp, name)
    k = np.concatenate([sp, random_bits(sp.dtype, 500, rng), sp[::-1], e])
    run_range(dev, name, k, e)
    run_range(dev, name, k, e[3:-2])                                   # some special keys outside the edges
    run_range(dev, name, k, sort_edges(np.concatenate([sp[:4], sp[:4]]), name))   # special edges repeated
    if name[0] == "f":   # -0 and +0 are neighbours; the NaNs lie outside the infinities
        w = sp.dtype.itemsize
        nz, pz = sp.dtype.type(1 << (8 * w - 1)), sp.dtype.type(0)
        ninf, pinf = (sp[9], sp[8])
        res = run_range(dev, name, k, np.array([ninf, nz, pz, pinf], dtype=sp.dtype))
        code = encode(k, name)
        c = lambda b: int(encode(np.array([b], dtype=sp.dtype), name)[0])   # noqa: E731
        assert res[0][1] == np.count_nonzero(k == nz) and int(res[1].sum()) == np.count_nonzero((code >= c(ninf)) & (code <= c(pinf)))


def test_range_all_keys_in_one_bin(dev):
    """70 000 adds to one counter: more than 16 bits hold, and no same-address add may be lost"""
    n = 70000
    e = np.array([10, 20, 30, 40], dtype=np.uint32)
    k = np.full(n, 25, dtype=np.uint32)
    for grid in (0, 1):
        res = run_range(dev, "u32", k, e, grid=grid)
        assert res[0].tolist() == [0, n, 0]
    k64 = np.full(n, np.float64(-2.5).view(np.uint64), dtype=np.uint64)
    e64 = np.array([-3.0, -2.5, -2.0], dtype=np.float64).view(np.uint64)
    assert run_range(dev, "f64", k64, e64, grid=1)[1].tolist() == [0, n]


def test_range_alternating_keys_over_two_bins(dev):
    n = 3 * T + 5
    k = np.where(np.arange(n) % 2 == 0, np.int32(-7), np.int32(7)).astype(np.int32).view(np.uint32)
    e = np.array([-100, 0, 100], dtype=np.int32).view(np.uint32)
    for grid in (0, 2):
        assert run_range(dev, "i32", k, e, grid=grid)[0].tolist() == [(n + 1) // 2, n // 2]


# ---------------------------------------------------------------------------------------------
# bincount
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["1", "2", "1000", "limit", "limit+1"])
@pytest.mark.parametrize("name", INT_IDS)
def test_bincount_types_and_bin_counts(dev, lds_limit, name, which):
    assert lds_limit >= 8192
    bins = {"1": 1, "2": 2, "1000": 1000, "limit": lds_limit, "limit+1": lds_limit + 1}[which]
    n = 100000 if which == "limit+1" else 5000   # limit + 1: the sorted path, no knob
    rng = np.random.default_rng(bins + BY_NAME[name][1])
    got = run_bincount(dev, name, int_keys(name, n, bins, rng), bins)
    assert 0 < int(got.sum()) < n


@pytest.mark.parametrize("bins", [65, 1000])
@pytest.mark.parametrize("n", [1, 5000])
@pytest.mark.parametrize("name", INT_IDS)
def test_bincount_sorted_path_equals_lds_path(dev, name, n, bins):
    rng = np.random.default_rng(n + bins + BY_NAME[name][1])
    k = int_keys(name, n, bins, rng)
    if n == 1:
        k[0] = bins - 1
    sorted_path = run_bincount(dev, name, k, bins, lds_bins=64)
    lds_path = run_bincount(dev, name, k, bins)
    assert np.array_equal(sorted_path, lds_path)
    if n == 1:   # and a single key out of range, negative where the type has a sign
        k[0] = np.array([-1], dtype=np.int64).astype(BY_NAME[name][2]).view(BY_NAME[name][3])[0]
        assert run_bincount(dev, name, k, bins, lds_bins=64).sum() == 0 and run_bincount(dev, name, k, bins).sum() == 0


def test_bincount_int64_keys_above_2_to_32(dev):
    bins = 1000
    k = np.concatenate([np.arange(bins, dtype=np.int64) + (1 << 32), np.arange(bins, dtype=np.int64) * (1 << 32), np.arange(7, dtype=np.int64),
                        -np.arange(1, 9, dtype=np.int64)]).view(np.uint64)
    want = np.zeros(bins, np.uint32)
    want[:7] = 1
    want[0] += 1
    for lds_bins in (0, 64):
        assert np.array_equal(run_bincount(dev, "i64", k, bins, lds_bins=lds_bins), want)


def test_bincount_sorted_path_on_descending_and_on_all_equal_keys(dev):
    """the sort has work to do; then one run that spans the whole input"""
    rng = np.random.default_rng(9)
    bins = 300
    k = np.sort(int_keys("u32", 3 * T + 1, bins, rng))[::-1].copy()
    run_bincount(dev, "u32", k, bins, lds_bins=1)
    run_bincount(dev, "u32", np.full(4097, 5, np.uint32), bins, lds_bins=1)


# ---------------------------------------------------------------------------------------------
# memory contract
# ---------------------------------------------------------------------------------------------
def test_work_prefilled_and_repeated_calls_give_the_same_counts(dev):
    rng = np.random.default_rng(12)
    n = 2 * T + 77
    e = edges_of("f64", 300, rng, "repeated")
    k = keys_for("f64", n, e, rng)
    ki = int_keys("i32", n, 500, rng)
    a = run_range(dev, "f64", k, e, grid=5)
    b = run_range(dev, "f64", k, e, grid=5, fill=0xff)
    assert all(np.array_equal(a[u], b[u]) for u in (0, 1))
    for lds_bins in (0, 64):
        assert np.array_equal(run_bincount(dev, "i32", ki, 500, lds_bins=lds_bins), run_bincount(dev, "i32", ki, 500, lds_bins=lds_bins, fill=0xff))
    c = Case(dev, "f64", k, e, 300, fill=0xff)
    try:
        for _ in range(2):   # the same call twice on one work buffer, without clearing anything in between
            assert c.call(1) == 0, lib_err()
            assert np.array_equal(c.check(histogram_range_oracle(k, "f64", e, True), "repeat"), a[1])
            c.reset()
    finally:
        c.release()


@pytest.mark.parametrize("mode", ["range", "bincount_lds", "bincount_sorted"])
def test_work_buffer_one_byte_short_is_refused(dev, mode):
    rng = np.random.default_rng(13)
    n = T + 1
    if mode == "bincount_sorted":
        dev.setParam("debug.histogram_lds_bins", 64)
    try:
        if mode == "range":
            e = edges_of("i32", 70, rng)
            c = Case(dev, "i32", keys_for("i32", n, e, rng), e, 70)
        else:
            c = Case(dev, "i32", int_keys("i32", n, 70, rng), None, 70)
        try:
            need = c.work.nbytes
            assert need > 0
            assert c.call(work_bytes=need - 1) == 1
            assert ("work buffer too small: %d < %d" % (need - 1, need)) in lib_err()
            c.untouched()
            assert c.call(work_bytes=need) == 0, lib_err()
        finally:
            c.release()
    finally:
        dev.setParam("debug.histogram_lds_bins", 0)


def test_refusals_come_before_anything_is_enqueued(dev):
    lib = _lib.load()
    rng = np.random.default_rng(14)
    n = 100
    e = edges_of("f32", 16, rng)
    c = Case(dev, "f32", keys_for("f32", n, e, rng), e, 16)
    ci = Case(dev, "i64", int_keys("i64", n, 16, rng), None, 16)
    h, kp, ep, cp, wp, wb = dev._h, c.keys.ptr(), c.edges.ptr(), c.counts.ptr(), c.work.ptr(), c.work.nbytes
    try:
        bad = [
            lib.adlhip_histogram_range_typed(h, 2, None, n, ep, 16, 0, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, None, 16, 0, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, None, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, cp, None, wb),
            lib.adlhip_histogram_range_typed(h, 2, c.keys.ptr(4), n - 1, ep, 16, 0, cp, wp, wb),     # misaligned
            lib.adlhip_histogram_range_typed(h, 2, kp, n, c.edges.ptr(4), 15, 0, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, c.counts.ptr(4), wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, cp, c.work.ptr(4), wb - 4),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, kp, wp, wb),                    # the counters over the keys
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 0, c.edges.ptr(16), wp, wb),       # ... over the edges
            lib.adlhip_histogram_range_typed(h, 6, kp, n, ep, 16, 0, cp, wp, wb),                    # key type
            lib.adlhip_histogram_range_typed(h, -1, kp, n, ep, 16, 0, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 0, 0, cp, wp, wb),                     # num_bins
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, HISTOGRAM_MAX_RANGE_BINS + 1, 0, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, 2, cp, wp, wb),                    # include_upper
            lib.adlhip_histogram_range_typed(h, 2, kp, n, ep, 16, -1, cp, wp, wb),
            lib.adlhip_histogram_range_typed(h, 2, kp, 1 << 32, ep, 16, 0, cp, wp, wb),              # n
        ]
        assert bad == [1] * len(bad), bad
        c.untouched()
        kp, cp, wp, wb = ci.keys.ptr(), ci.counts.ptr(), ci.work.ptr(), ci.work.nbytes
        bad = [
            lib.adlhip_bincount_typed(h, 4, None, n, 16, cp, wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 16, None, wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 16, cp, None, wb),
            lib.adlhip_bincount_typed(h, 4, ci.keys.ptr(8), n - 1, 16, cp, wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 16, ci.counts.ptr(4), wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 16, kp, wp, wb),
            lib.adlhip_bincount_typed(h, 2, kp, n, 16, cp, wp, wb),                                  # float keys
            lib.adlhip_bincount_typed(h, 5, kp, n, 16, cp, wp, wb),
            lib.adlhip_bincount_typed(h, 6, kp, n, 16, cp, wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 0, cp, wp, wb),
            lib.adlhip_bincount_typed(h, 4, kp, n, 1 << 31, cp, wp, wb),
        ]
        assert bad == [1] * len(bad), bad
        assert "num_bins must be in" in lib_err()
        ci.untouched()
        sz = ctypes.c_size_t()
        assert lib.adlhip_histogram_scratch_bytes(h, 2, n, 16, 0, ctypes.byref(sz)) == 1      # bincount of floats
        assert lib.adlhip_histogram_scratch_bytes(h, 2, n, 4097, 1, ctypes.byref(sz)) == 1
        assert lib.adlhip_histogram_scratch_bytes(h, 1, n, 16, 2, ctypes.byref(sz)) == 1
    finally:
        c.release()
        ci.release()


def test_empty_input_clears_the_counters_and_looks_at_nothing_else(dev):
    """n == 0: one clear of the counters; the keys, the work buffer and its size are not looked at, everything else is"""
    lib = _lib.load()
    e = np.array([1, 2, 3, 4], dtype=np.uint32)
    c = Case(dev, "u32", np.zeros(0, np.uint32), e, 3)
    h, ep, cp = dev._h, c.edges.ptr(), c.counts.ptr()
    try:
        assert lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 3, 1, cp, None, 0) == 0, lib_err()
        assert c.counts.read(np.uint32).tolist() == [0, 0, 0]
        c.reset()
        assert lib.adlhip_bincount_typed(h, 0, None, 0, 3, cp, None, 0) == 0, lib_err()
        assert c.counts.read(np.uint32).tolist() == [0, 0, 0]
        c.reset()
        bad = [lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 3, 1, None, None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 3, 1, c.counts.ptr(4), None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, None, 3, 1, cp, None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, c.edges.ptr(4), 2, 1, cp, None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 3, 2, cp, None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 0, 0, cp, None, 0),
               lib.adlhip_histogram_range_typed(h, 0, None, 0, ep, 3, 0, ep, None, 0),
               lib.adlhip_bincount_typed(h, 2, None, 0, 3, cp, None, 0),
               lib.adlhip_bincount_typed(h, 0, None, 0, 0, cp, None, 0),
               lib.adlhip_bincount_typed(h, 0, None, 0, 3, None, None, 0)]
        assert bad == [1] * len(bad), bad
        c.untouched()
    finally:
        c.release()


def test_scratch_is_modest_and_independent_of_n_on_the_lds_path(dev, lds_limit):
    cus = DeviceUtils.getNCUs(dev)
    for name, bins, by_edges in (("f64", 4096, 1), ("i32", 256, 0), ("i64", lds_limit, 0)):
        a, b = scratch_bytes(dev, name, 1000, bins, by_edges), scratch_bytes(dev, name, 1 << 26, bins, by_edges)
        assert a == b and a % 256 == 0 and a <= 64 << 20
        g = min(max(4 * cus * 2048 // bins, 2 * cus), 4 * cus)   # the formula of the header
        assert a == (g * bins * 4 + 255) // 256 * 256
    assert scratch_bytes(dev, "i32", 1 << 20, lds_limit + 1, 0) >= 2 * 4 << 20   # the sorted path holds two copies of the keys


# ---------------------------------------------------------------------------------------------
# the torch front end
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter()
    yield s
    s.close()


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_torch_bincount(sorter, dtype):
    g = torch.Generator(device="cpu").manual_seed(1)
    for hi, n in ((7, 1), (300, 5 * T + 3), (20000, 30000)):   # 20000 values: above the LDS limit
        t = torch.randint(0, hi, (n,), generator=g).to(dtype).cuda()
        got = sorter.bincount(t)
        want = torch.bincount(t)
        assert got.dtype == torch.int64 and torch.equal(got, want)
        assert torch.equal(sorter.bincount(t, num_bins=hi + 5), torch.bincount(t, minlength=hi + 5)[:hi + 5])
        assert torch.equal(sorter.bincount(t, num_bins=3), want[:3] if want.numel() >= 3 else torch.bincount(t, minlength=3))
    assert sorter.bincount(torch.empty(0, dtype=dtype, device="cuda")).numel() == 0
    assert sorter.bincount(torch.empty(0, dtype=dtype, device="cuda"), num_bins=4).tolist() == [0, 0, 0, 0]
    neg = torch.tensor([-5, 2, 2, -1, 0], dtype=dtype, device="cuda")
    assert sorter.bincount(neg).tolist() == [1, 0, 2]
    for only_negative in ([-1], [-5, -2, -2]):   # max + 1 <= 0: no bins
        got = sorter.bincount(torch.tensor(only_negative, dtype=dtype, device="cuda"))
        assert got.dtype == torch.int64 and got.numel() == 0
    assert sorter.bincount(torch.tensor([-5, -2], dtype=dtype, device="cuda"), num_bins=2).tolist() == [0, 0]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.float32, torch.float64])
def test_torch_histogram_is_numpy_histogram(sorter, dtype):
    rng = np.random.default_rng(2)
    npdt = {torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32, torch.float64: np.float64}[dtype]
    v = (rng.standard_normal(3 * T + 11) * 40).astype(npdt)
    v[v == 0] = 0   # no -0
    for edges in (np.linspace(-100, 100, 34).astype(npdt), np.array([-50, -50, 0, 7, 7, 7, 120], dtype=npdt), np.array([3, 3], dtype=npdt)):
        v[::50] = edges[rng.integers(0, edges.size, size=v[::50].size)]
        got = sorter.histogram(torch.from_numpy(v).cuda(), torch.from_numpy(edges).cuda())
        assert got.dtype == torch.int64 and got.cpu().numpy().tolist() == np.histogram(v, bins=edges)[0].tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32])
def test_torch_histc_is_numpy_histogram_on_its_edges(sorter, dtype):
    rng = np.random.default_rng(3)
    npdt = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32}[dtype]
    v = (rng.random(2 * T + 5) * 120 - 10).astype(npdt)
    for bins, lo, hi in ((100, 0, 100), (7, -3, 50), (1, 0, 1), (4096, -10, 110)):
        edges = torch.linspace(lo, hi, bins + 1, dtype=torch.float64).to(dtype).numpy()
        got = sorter.histc(torch.from_numpy(v).cuda(), bins=bins, min=lo, max=hi)
        assert got.cpu().numpy().tolist() == np.histogram(v, bins=edges)[0].tolist(), (bins, lo, hi)
    # min == max: the tensor's own range
    edges = torch.linspace(float(v.min()), float(v.max()), 11, dtype=torch.float64).to(dtype).numpy()
    assert sorter.histc(torch.from_numpy(v).cuda(), bins=10).cpu().numpy().tolist() == np.histogram(v, bins=edges)[0].tolist()


def test_torch_histc_keys_on_the_edges(sorter):
    """exact multiples of the bin width land on edges: each belongs to the bin it opens, the last edge to the last bin"""
    bins, width = 40, 0.25
    v = (np.arange(0, bins + 1, dtype=np.float32) * np.float32(width)).repeat(3)
    v = np.concatenate([v, np.float32([-width, (bins + 1) * width])])
    got = sorter.histc(torch.from_numpy(v).cuda(), bins=bins, min=0.0, max=bins * width).cpu().numpy()
    edges = torch.linspace(0.0, bins * width, bins + 1, dtype=torch.float64).to(torch.float32).numpy()
    want = histogram_range_oracle(v.view(np.uint32), "f32", edges.view(np.uint32), True)
    assert got.tolist() == want.tolist() and got.tolist() == [3] * (bins - 1) + [6]


def test_torch_views_at_odd_offsets_and_refusals(sorter):
    base = torch.arange(0, 4001, dtype=torch.int32, device="cuda") % 50
    view = base[1:]          # starts 4 bytes behind a 16-byte boundary
    assert view.data_ptr() % 16 != 0
    assert torch.equal(sorter.bincount(view, num_bins=50), torch.bincount(view, minlength=50))
    fbase = torch.linspace(-1, 2, 3003, dtype=torch.float64, device="cuda")
    fview, eview = fbase[1::2], torch.linspace(0, 1, 12, dtype=torch.float64, device="cuda")[1:]
    assert sorter.histogram(fview, eview).cpu().numpy().tolist() == np.histogram(fview.cpu().numpy(), bins=eview.cpu().numpy())[0].tolist()
    assert torch.equal(base, torch.arange(0, 4001, dtype=torch.int32, device="cuda") % 50)
    t = torch.arange(10, dtype=torch.int32, device="cuda")
    e = torch.arange(4, dtype=torch.int32, device="cuda")
    for bad in (t.to(torch.float16), t.to(torch.uint8), [1, 2, 3]):
        with pytest.raises(TypeError):
            sorter.bincount(bad)
        with pytest.raises(TypeError):
            sorter.histc(bad, 4, 0, 1)
    with pytest.raises(TypeError):
        sorter.histogram(t, [0, 1, 2])
    with pytest.raises(TypeError):
        sorter.bincount(t.to(torch.float32))
    with pytest.raises(TypeError):
        sorter.histogram(t, e.to(torch.int64))
    with pytest.raises(ValueError):
        sorter.bincount(t.cpu())
    with pytest.raises(ValueError):
        sorter.histogram(t, e.cpu())
    with pytest.raises(ValueError):
        sorter.histogram(t.reshape(2, 5), e)
    with pytest.raises(ValueError):
        sorter.histogram(t, e[:1])
    with pytest.raises(ValueError):
        sorter.histc(t, 0, 0, 1)
    with pytest.raises(ValueError):
        sorter.histc(t, 4097, 0, 1)
    with pytest.raises(ValueError):
        sorter.histc(t, 4, 2, 1)
    with pytest.raises(ValueError):
        sorter.bincount(t, num_bins=-1)


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def test_histogram_demo_on_the_device_matches_the_oracle():
    assert os.path.exists(DEMO)
    r = subprocess.run([DEMO, "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    check_demo_output(r.stdout)
