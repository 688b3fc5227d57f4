"""The memory side of the C ABI's contract (include/adlhip.h), checked on the GPU.

A sort writes only d_keys_inout[0, n), d_tmp[0, n) and d_work[0, work_bytes) (SoA sorts: the two tmp arrays too); a partition
writes its output, counts[num_buckets] / totals256[256] and its work, never its input; a scan writes dst[0, n).  The work
buffer's contents on entry are arbitrary, buffers need only 16-byte alignment, and the size adlhip_radix_sort_scratch_bytes(N)
reports suffices for every n' <= N.

Every region a call may touch sits in one larger adlhip_malloc allocation (the "arena") between two guard bands that are filled
with known bytes before the call and compared byte for byte after it.  The band after a data array doubles as poison: keys 0 and
~0 alternate there, so an over-read that feeds them into the result changes the result.  Regions start at 0 or 16 (mod 256);
scratch interiors start as 0xFF bytes (status words then read as "prefix available", tickets as huge) or as random bytes.
Results are compared bit-exactly with a plain host reference (numpy / the oracle).  Everything goes through the C ABI so that
the test chooses every pointer and byte count.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
from oclradixsort_amd import DeviceUtils, _lib
from oclradixsort_amd._lib import check

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
Mi = 1 << 20
BEFORE_BAND = 64 * KiB
POOL_BYTES = 128 * MiB + 4096
K_MAX_ELEMS = 0xFFF00000
MARKER = 0xB0BAFE77          # the value half of poison pairs

U32, KV32, U64, SOA32 = 0, 1, 2, 3
KIND_NAME = {U32: "u32", KV32: "kv32", U64: "u64", SOA32: "soa32"}
ESZ = {U32: 4, KV32: 8, U64: 8, SOA32: 4}
MAX_BITS = {U32: 32, KV32: 32, U64: 64, SOA32: 32}

DEFAULT_KNOBS = {"sort.algo": -1, "sort.digit_bits": 8, "sort.tile": -1, "sort.msd2": 1, "sort.mid": 1, "sort.dict": 1,
                 "sort.binfinish": 1, "sort.net_lookback": 1, "partition.lookback": 1}

# what the module ran: union of profile labels, net statistics per family, forms along the in-between sweeps
SEEN_LABELS = set()
NET_FAMILIES = set()
SWEEP_FORMS = {}


def align_up(x, a):
    return (x + a - 1) // a * a


def _lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


# ---------------------------------------------------------------------------------------------
# the guarded arena
# ---------------------------------------------------------------------------------------------
class _Pool:
    """128 MiB of seeded random bytes; a band of region r of case c is a slice at an offset derived from (c, r), so every band
    differs from its neighbours and a block copied from one region into another is recognisable."""
    _bytes = None

    @classmethod
    def get(cls):
        if cls._bytes is None:
            cls._bytes = np.frombuffer(np.random.default_rng(20261016).bytes(POOL_BYTES), dtype=np.uint8)
        return cls._bytes

    @classmethod
    def slice(cls, seed, length):
        pool = cls.get()
        length = int(length)
        if length <= pool.size // 2:
            off = (seed * 1048573 * 16) % (pool.size - length)
            return pool[off:off + length]
        reps = -(-length // pool.size)
        return np.tile(pool, reps)[:length]


def poison_bytes(kind, nbytes):
    """Alternating all-zero / all-ones keys (pairs: with the marker value) -- what an over-read would feed into the result."""
    if kind in (U32, "u32v"):
        pat = np.array([0, 0xFFFFFFFF], dtype=np.uint32)
    elif kind == KV32:
        pat = np.array([MARKER << 32, (MARKER << 32) | 0xFFFFFFFF], dtype=np.uint64)
    elif kind == U64:
        pat = np.array([0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    else:
        raise ValueError(kind)
    b = pat.view(np.uint8)
    return np.tile(b, -(-nbytes // b.size))[:nbytes]


class Arena:
    """One device allocation, grown on demand and reused by every case of the module."""

    def __init__(self, dev):
        self.dev = dev
        self.base = 0
        self.size = 0

    def ensure(self, nbytes):
        if nbytes <= self.size:
            return
        self.release()
        size = align_up(nbytes, 64 * MiB)
        p = ctypes.c_void_p()
        check(_lib.load().adlhip_malloc(self.dev._h, size, ctypes.byref(p)), "adlhip_malloc(arena)")
        self.base, self.size = p.value, size

    def release(self):
        if self.base:
            check(_lib.load().adlhip_free(self.dev._h, ctypes.c_void_p(self.base), self.size), "adlhip_free(arena)")
        self.base = self.size = 0


class Region:
    def __init__(self, layout, name, off, nbytes, before_off, after_len, after_bytes, seed):
        self.layout, self.name, self.off, self.nbytes = layout, name, off, nbytes
        self.before_off, self.after_len, self.seed = before_off, after_len, seed
        self.before_expect = _Pool.slice(seed, off - before_off)
        self.after_expect = after_bytes if after_bytes is not None else _Pool.slice(seed + 7777, after_len)

    @property
    def addr(self):
        return self.layout.arena.base + self.off

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)


def after_band_bytes(nbytes):
    return align_up(max(MiB, min(nbytes // 8, 64 * MiB)), 16)


class Layout:
    """Regions of one call, each between a band of >= 64 KiB before and max(1 MiB, min(size / 8, 64 MiB)) after it; the after
    band starts at the region's exact end.  Region j of case c starts at 16 * ((c + j) % 2) (mod 256) unless told otherwise."""

    def __init__(self, arena, case_no):
        self.arena, self.case_no = arena, case_no
        self.regions = []
        self.cursor = 0
        self.keep = []

    def add(self, name, nbytes, poison=None, shift=None):
        j = len(self.regions)
        if shift is None:
            shift = 16 * ((self.case_no + j) % 2)
        before_off = self.cursor
        off = align_up(before_off + BEFORE_BAND, 256) + shift
        after_len = after_band_bytes(nbytes)
        after = poison_bytes(poison, after_len) if poison is not None else None
        r = Region(self, name, off, int(nbytes), before_off, after_len, after, seed=self.case_no * 131 + j * 17 + 1)
        self.regions.append(r)
        self.cursor = align_up(off + nbytes + after_len, 256)
        return r

    def commit(self):
        """Allocate and write every band (the region interiors are the caller's)."""
        self.arena.ensure(self.cursor)
        lib, h = _lib.load(), self.arena.dev._h
        for r in self.regions:
            for off, data in ((r.before_off, r.before_expect), (r.off + r.nbytes, r.after_expect)):
                data = np.ascontiguousarray(data)
                self.keep.append(data)
                check(lib.adlhip_memcpy_h2d(h, ctypes.c_void_p(self.arena.base + off), data.ctypes.data_as(ctypes.c_void_p), data.nbytes), "h2d band")
        sync(self.arena.dev)
        self.keep = []

    def upload(self, region, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= region.nbytes, (region.name, arr.nbytes, region.nbytes)
        check(_lib.load().adlhip_memcpy_h2d(self.arena.dev._h, ctypes.c_void_p(region.addr + offset), arr.ctypes.data_as(ctypes.c_void_p),
                                            arr.nbytes), "h2d")
        self.keep.append(arr)

    def prefill(self, region, mode):
        """Scratch interior: 0xFF bytes, or seeded random bytes."""
        lib, h = _lib.load(), self.arena.dev._h
        if mode == "ff" or region.nbytes == 0:
            check(lib.adlhip_memset(h, region.ptr, 0xFF, region.nbytes), "memset")
            return
        src = _Pool.slice(region.seed + 31, min(region.nbytes, 32 * MiB))
        done = 0
        while done < region.nbytes:
            k = min(src.size, region.nbytes - done)
            check(lib.adlhip_memcpy_h2d(h, ctypes.c_void_p(region.addr + done), src.ctypes.data_as(ctypes.c_void_p), k), "h2d")
            done += k
        self.keep.append(src)

    def read(self, off, nbytes, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes:
            check(_lib.load().adlhip_memcpy_d2h(self.arena.dev._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.arena.base + off),
                                                nbytes), "d2h")
        return out

    def fetch(self, region, dtype, count=None):
        nb = region.nbytes if count is None else count * np.dtype(dtype).itemsize
        out = self.read(region.off, nb, dtype)
        sync(self.arena.dev)
        return out

    def band_damage(self):
        """[(region, side, first, last, count, found sample, expected sample)] of every band that changed."""
        got = []
        for r in self.regions:
            got.append((r, "before", r.before_off, r.before_expect, self.read(r.before_off, r.off - r.before_off)))
            got.append((r, "after", r.off + r.nbytes, r.after_expect, self.read(r.off + r.nbytes, r.after_len)))
        sync(self.arena.dev)
        bad = []
        for r, side, start, want, have in got:
            diff = np.flatnonzero(have != want)
            if diff.size:
                # offsets are relative to the region start (negative: inside the band before it)
                rel = start - r.off
                bad.append((r.name, side, int(diff[0]) + rel, int(diff[-1]) + rel, int(diff.size),
                            have[diff[:8]].tolist(), want[diff[:8]].tolist()))
        return bad

    def assert_bands_intact(self, what):
        bad = self.band_damage()
        assert not bad, "%s: guard bands changed (region, side, first offset, last offset, bytes, found, expected): %s" % (what, bad)

    def snapshot(self):
        img = self.read(0, self.cursor)
        sync(self.arena.dev)
        return img


def sync(dev):
    rc = _lib.load().adlhip_sync(dev._h)
    assert rc == 0, "adlhip_sync reported: %s" % _lib_err()


# ---------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    d.toggleProfiling(True)
    yield d
    d.toggleProfiling(False)
    DeviceUtils.deallocate(d)


@pytest.fixture(scope="module")
def arena(dev):
    a = Arena(dev)
    yield a
    a.release()


@pytest.fixture(autouse=True)
def _default_knobs(request):
    if "dev" in request.fixturenames:
        d = request.getfixturevalue("dev")
        set_knobs(d, {})
    yield
    if "dev" in request.fixturenames:
        set_knobs(request.getfixturevalue("dev"), {})


def set_knobs(dev, knobs):
    for k, v in DEFAULT_KNOBS.items():
        dev.setParam(k, knobs.get(k, v))
    dev.setParam("sort.rank", knobs.get("sort.rank", dev.getParam("sort.lds_ordered")))


def net_stats(dev):
    return dev.getParam("stat.net_runs"), dev.getParam("stat.net_counting")


def run_profiled(dev, fn):
    """fn() -> rc; returns (rc, labels, (net runs, net counting) deltas).  Reading the profile waits for the stream."""
    dev.profile(reset=True)
    r0, c0 = net_stats(dev)
    rc = fn()
    labels = set(dev.profile(reset=True))
    r1, c1 = net_stats(dev)
    SEEN_LABELS.update(labels)
    return rc, labels, (r1 - r0, c1 - c0)


def scratch_for(dev, kind, n, bits, level):
    tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    check(_lib.load().adlhip_radix_sort_scratch_bytes_for(dev._h, kind, n, bits, level, ctypes.byref(tb), ctypes.byref(wb)), "scratch_bytes_for")
    return tb.value, wb.value


# ---------------------------------------------------------------------------------------------
# inputs and host references
# ---------------------------------------------------------------------------------------------
def make_keys(width, n, dist, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint32 if width == 32 else np.uint64
    top = np.uint64(0xFFFFFFFFFFFFFFFF) if width == 64 else np.uint32(0xFFFFFFFF)
    if dist == "uniform":
        return oracle.keys_u32(n, seed=seed) if width == 32 else oracle.keys_u64(n, seed=seed)
    if dist in ("few256", "dict4096"):
        d = 256 if dist == "few256" else 4096
        vals = rng.integers(1, int(top), d, dtype=dt, endpoint=False)
        vals[0], vals[1] = 0, top           # 0 and the all-ones key among them
        return vals[rng.integers(0, d, n)]
    if dist == "heavy":                     # one top byte holds ~90 % of the keys, the bits below vary
        k = oracle.keys_u32(n, seed=seed) if width == 32 else oracle.keys_u64(n, seed=seed)
        sel = rng.random(n) < 0.9
        if width == 32:
            k[sel] = (k[sel] & np.uint32(0x00FFFFFF)) | np.uint32(0x5A000000)
        else:
            k[sel] = (k[sel] & np.uint64(0x00FFFFFFFFFFFFFF)) | np.uint64(0x5A << 56)
        return k
    if dist == "sorted":
        return np.sort(oracle.keys_u32(n, seed=seed) if width == 32 else oracle.keys_u64(n, seed=seed))
    raise ValueError(dist)


def stable_order(keys, bits):
    """Indices of the stable sort by the low `bits` bits of the keys."""
    n = keys.size
    if keys.dtype == np.uint32 or bits <= 32:
        low = keys.astype(np.uint64) & np.uint64((1 << bits) - 1)
        if n < (1 << 32) and bits <= 32:
            return (np.sort((low << np.uint64(32)) | np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    low = keys & np.uint64((1 << bits) - 1) if bits < 64 else keys
    if bits + max(1, int(n - 1).bit_length()) <= 64:
        sh = np.uint64(64 - bits)
        return (np.sort((low << sh) | np.arange(n, dtype=np.uint64)) & np.uint64((1 << (64 - bits)) - 1)).astype(np.int64)
    return np.argsort(low, kind="stable")


# ---------------------------------------------------------------------------------------------
# the sort matrix
# ---------------------------------------------------------------------------------------------
KNOB_SETS = [
    ("default", {}),
    ("onesweep4", {"sort.algo": 0, "sort.digit_bits": 4}),
    ("onesweep8", {"sort.algo": 0}),
    ("threekernel", {"sort.algo": 1}),
    ("rank0", {"sort.rank": 0}),
    ("msd2forced", {"sort.msd2": 2}),
    ("msd2stable", {"sort.msd2": 3}),
    ("msd2cursor", {"sort.msd2": 4}),
    ("msd2hybrid", {"sort.msd2": 5}),
    ("mid0", {"sort.mid": 0}),
]
KNOBS = dict(KNOB_SETS, mid2={"sort.mid": 2}, mid3={"sort.mid": 3})
LEVELS = [0, 2, 1]
MAX_BITS_BY_NAME = {"u32": 32, "kv32": 32, "u64": 64, "soa32": 32}


def _sort_cases():
    sizes = {
        "u32": [1, 3, 4097, 16383, 16384, 16385, 65537, Mi + 1, 2 * Mi - 1, 2 * Mi + 1, 6 * Mi + 3, 12 * Mi + 1, 16 * Mi - 1, 16 * Mi + 1,
                20 * Mi + 77],
        "kv32": [1, 4097, 16385, Mi - 1, Mi + 1, 4 * Mi + Mi // 2 + 1, 8 * Mi + 77, 16 * Mi + 1],
        "u64": [3, 16385, Mi + 1, 3 * Mi + 17, 16 * Mi + 1],
        "soa32": [4097, Mi + 1, 4 * Mi + 11, 16 * Mi + 3],
    }
    partial = {"u32": [20, 28], "kv32": [24], "u64": [40, 44], "soa32": [24]}
    cases = []
    i = 0
    for kind, ns in sizes.items():
        for j, n in enumerate(ns):
            dists = ["uniform", "few256", "dict4096" if kind == "u32" else None, "heavy", "sorted"] if n >= Mi else ["uniform", "few256"]
            for dist in [x for x in dists if x]:
                knob = KNOB_SETS[i % len(KNOB_SETS)][0]
                extra = {}
                if dist == "heavy":
                    extra = {"sort.net_lookback": (i // 3) % 2}
                cases.append((kind, n, dist, MAX_BITS_BY_NAME[kind], LEVELS[i % 3], knob, extra))
                i += 1
            if n >= 2 * Mi:      # every size from 2 Mi: the minimum and the full-speed scratch on uniform keys, default knobs
                cases.append((kind, n, "uniform", MAX_BITS_BY_NAME[kind], 0, "default", {}))
                cases.append((kind, n, "uniform", MAX_BITS_BY_NAME[kind], 1, "default", {}))
            if n >= 4097 and (kind != "u64" or n <= 3 * Mi + 17):
                bits = partial[kind][j % len(partial[kind])]
                knob = KNOB_SETS[i % len(KNOB_SETS)][0]
                cases.append((kind, n, "uniform", bits, LEVELS[i % 3], knob, {}))
                i += 1
    # the largest sizes: uniform keys only
    cases += [("u32", 64 * Mi + 12345, "uniform", 32, 1, "default", {}), ("u32", 64 * Mi + 12345, "uniform", 32, 2, "default", {}),
              ("u32", 150 * Mi + 3, "uniform", 32, 1, "default", {}), ("u32", 150 * Mi + 3, "uniform", 32, 0, "default", {}),
              ("kv32", 64 * Mi, "uniform", 32, 1, "default", {}), ("kv32", 64 * Mi, "uniform", 32, 2, "msd2stable", {}),
              ("u64", 32 * Mi + 5, "uniform", 64, 1, "msd2stable", {}), ("u64", 32 * Mi + 5, "uniform", 64, 0, "default", {})]
    # paths the rotation above need not reach: both mid-size forms, the stable large sort of u64 keys on part of the key, the
    # safety net's counting sorts and its two kinds of LSD passes
    cases += [("u32", 300007, "uniform", 32, 1, "mid2", {}), ("u32", 300007, "uniform", 32, 1, "mid3", {}),
              ("kv32", 300007, "uniform", 32, 1, "mid3", {}), ("u64", 3 * Mi + 17, "uniform", 40, 1, "default", {}),
              ("u32", 6 * Mi + 3, "few256", 32, 1, "default", {}), ("u32", 6 * Mi + 3, "dict4096", 32, 1, "default", {}),
              ("u64", 3 * Mi + 17, "few256", 64, 1, "default", {}),
              ("u32", 6 * Mi + 3, "heavy", 32, 1, "default", {"sort.net_lookback": 1}),
              ("u32", 6 * Mi + 3, "heavy", 32, 2, "default", {"sort.net_lookback": 0})]
    return cases


SORT_CASES = _sort_cases()


def _case_id(c):
    kind, n, dist, bits, level, knob, extra = c
    s = "%s-n%d-%s-b%d-L%d-%s" % (kind, n, dist, bits, level, knob)
    for k, v in extra.items():
        s += "-%s%d" % (k.split(".")[-1], v)
    return s


def _one_sweep_knobs(knobs):
    return knobs.get("sort.algo") == 0


def sort_call(dev, kind, regs, work_bytes, n, bits):
    lib, h = _lib.load(), dev._h
    if kind == U32:
        return lib.adlhip_radix_sort_u32(h, regs["data"].ptr, regs["tmp"].ptr, regs["work"].ptr, work_bytes, n, bits)
    if kind == KV32:
        return lib.adlhip_radix_sort_kv32(h, regs["data"].ptr, regs["tmp"].ptr, regs["work"].ptr, work_bytes, n, bits)
    if kind == U64:
        return lib.adlhip_radix_sort_u64(h, regs["data"].ptr, regs["tmp"].ptr, regs["work"].ptr, work_bytes, n, bits)
    return lib.adlhip_radix_sort_soa32(h, regs["data"].ptr, regs["vals"].ptr, regs["tmp"].ptr, regs["tmpv"].ptr, regs["work"].ptr,
                                       work_bytes, n, bits)


class SortRun:
    """Input, guarded regions and host reference of one sort; run() sorts it and checks the result and every band."""

    def __init__(self, dev, arena, case_no, kind, n, dist, bits, tmp_n=None):
        self.dev, self.arena, self.kind, self.n, self.bits = dev, arena, kind, n, bits
        seed = (n * 2654435761 + case_no) & 0xFFFFFFFF
        width = 64 if kind == U64 else 32
        self.keys = make_keys(width, n, dist, seed)
        idx = np.arange(n, dtype=np.uint64)
        if kind == KV32:
            self.input = self.keys.astype(np.uint64) | (idx << np.uint64(32))
        elif kind == SOA32:
            self.input = self.keys
            self.vals = idx.astype(np.uint32)
        else:
            self.input = self.keys
        self.tmp_n = n if tmp_n is None else tmp_n      # tmp sized for a larger batch (scratch sized once)
        self._want = None

    def want(self):
        if self._want is None:
            k, bits = self.kind, self.bits
            if k in (U32, U64) and bits == MAX_BITS[k]:
                self._want = (np.sort(self.keys),)
            else:
                order = stable_order(self.keys, bits)
                if k == SOA32:
                    self._want = (self.keys[order], self.vals[order])
                else:
                    self._want = (self.input[order],)
        return self._want

    def layout(self, case_no, work_bytes, fill="ff"):
        esz = ESZ[self.kind]
        L = Layout(self.arena, case_no)
        poison = U32 if esz == 4 else (KV32 if self.kind == KV32 else U64)
        regs = {"data": L.add("data", self.n * esz, poison=poison)}
        if self.kind == SOA32:
            regs["vals"] = L.add("vals", self.n * 4, poison="u32v")
        regs["tmp"] = L.add("tmp", self.tmp_n * esz)
        if self.kind == SOA32:
            regs["tmpv"] = L.add("tmp_vals", self.tmp_n * 4)
        regs["work"] = L.add("work", work_bytes)
        L.commit()
        L.upload(regs["data"], self.input)
        if self.kind == SOA32:
            L.upload(regs["vals"], self.vals)
        for name in ("tmp", "tmpv", "work"):
            if name in regs:
                L.prefill(regs[name], fill)
        return L, regs

    def run(self, case_no, work_bytes, fill="ff", what="", expect_refusal=False):
        """expect_refusal: False = must sort; None = must sort exactly or be refused without touching memory."""
        L, regs = self.layout(case_no, work_bytes, fill)
        sync(self.dev)
        before = L.snapshot() if expect_refusal is not False else None
        rc, labels, net = run_profiled(self.dev, lambda: sort_call(self.dev, self.kind, regs, work_bytes, self.n, self.bits))
        if rc != 0:
            err = _lib_err()
            assert expect_refusal is not False, "%s: refused: %s" % (what, err)
            assert err, what
            sync(self.dev)
            assert np.array_equal(L.snapshot(), before), "%s: a refused call changed memory" % what
            return "refused", labels, net
        sync(self.dev)
        want = self.want()
        esz = ESZ[self.kind]
        got = L.fetch(regs["data"], np.uint32 if esz == 4 else np.uint64, self.n)
        if not np.array_equal(got, want[0]):
            bad = np.flatnonzero(got != want[0])
            raise AssertionError("%s: wrong result at %d positions, first %d: got %#x want %#x; bands: %s" % (
                what, bad.size, bad[0], int(got[bad[0]]), int(want[0][bad[0]]), L.band_damage()))
        if self.kind == SOA32:
            gv = L.fetch(regs["vals"], np.uint32, self.n)
            assert np.array_equal(gv, want[1]), "%s: values out of order" % what
        L.assert_bands_intact(what)
        return "sorted", labels, net


def _record_net(dist, knobs, net):
    runs, counting = net
    if counting > 0:
        NET_FAMILIES.add("net_counting_dict4096" if dist == "dict4096" else "net_counting")
    if runs - counting > 0:
        NET_FAMILIES.add("net_lsd_lookback" if knobs.get("sort.net_lookback", 1) else "net_lsd_count_scan_scatter")


@pytest.mark.parametrize("case", SORT_CASES, ids=[_case_id(c) for c in SORT_CASES])
def test_sort_stays_inside_its_buffers(dev, arena, case):
    kind_name, n, dist, bits, level, knob, extra = case
    kind = {"u32": U32, "kv32": KV32, "u64": U64, "soa32": SOA32}[kind_name]
    knobs = dict(KNOBS[knob], **extra)
    if level == 0 and _one_sweep_knobs(knobs):
        level = 1          # a level-0 buffer with one-sweep knobs is a refusal (test_refused_calls_leave_memory_untouched)
    set_knobs(dev, knobs)
    case_no = SORT_CASES.index(case)
    _, wb = scratch_for(dev, kind, n, bits, level)
    run = SortRun(dev, arena, case_no, kind, n, dist, bits)
    fill = "random" if case_no % 3 == 2 else "ff"
    status, labels, net = run.run(case_no, wb, fill=fill, what="%s (work %d, %s interior)" % (_case_id(case), wb, fill))
    assert status == "sorted"
    _record_net(dist, knobs, net)


# ---------------------------------------------------------------------------------------------
# scratch sizes: in-between work sizes, sized once for the largest batch, knobs changed after sizing
# ---------------------------------------------------------------------------------------------
def _form(labels):
    """A short name of the path a sort took, from its kernel labels."""
    if any(x.startswith("msd2h_") for x in labels):
        return "large-hybrid"
    if any(x.startswith("msd2s_pass") for x in labels):
        return "large-stable"
    if any(x.startswith("msd2_pass") for x in labels):
        return "large-cursor"
    if any(x.startswith("mid_") for x in labels):
        return "mid"
    if any(x.startswith("onesweep_") for x in labels):
        return "onesweep"
    if any(x.startswith("count_") for x in labels):
        return "threekernel"
    if any(x.startswith("small_sort") for x in labels):
        return "small"
    return "+".join(sorted(labels))


SWEEP_CONFIGS = [(U32, 3 * Mi + 5, 32), (U32, 15 * Mi + 7, 32), (U32, 20 * Mi + 77, 32), (U32, 20 * Mi + 77, 28), (KV32, 4 * Mi + 3, 32),
                 (U64, 3 * Mi + 17, 64)]


def _sweep_sizes(l0, l1, l2):
    geo = [int(round(l0 * (l1 / l0) ** (k / 13.0))) for k in range(1, 13)]
    sizes = [l0] + geo + [l2 - 1, l2, l2 + 1, l1 - 1, l1]
    return sorted(set(s for s in sizes if l0 <= s <= l1))


@pytest.mark.parametrize("cfg", SWEEP_CONFIGS, ids=["%s-n%d-b%d" % (KIND_NAME[c[0]], c[1], c[2]) for c in SWEEP_CONFIGS])
def test_work_sizes_between_the_levels(dev, arena, cfg):
    """Every work size between level 0 and level 1 sorts exactly and stays inside its buffers; the path changes along the sweep.
    Regression test for the lean stable form's fit check (sort_entry), which once used a different layout than msd2s_sort."""
    kind, n, bits = cfg
    key = "%s-n%d-b%d" % (KIND_NAME[kind], n, bits)
    run = None
    for msd2 in (1, 2):
        set_knobs(dev, {"sort.msd2": msd2})
        l0 = scratch_for(dev, kind, n, bits, 0)[1]
        l1 = scratch_for(dev, kind, n, bits, 1)[1]
        l2 = scratch_for(dev, kind, n, bits, 2)[1]
        assert l0 <= l2 <= l1, (l0, l2, l1)
        # whole u32 keys: the stable form's second slab holds 16-bit keys, so they need strictly less than a sort on 28 bits
        l2_28 = scratch_for(dev, kind, n, 28, 2)[1] - 1 if kind == U32 and bits == 32 else None
        if run is None:
            run = SortRun(dev, arena, 1000 + n % 97, kind, n, "uniform", bits)
        forms = []
        for i, wb in enumerate(sorted(set(_sweep_sizes(l0, l1, l2) + ([l2_28] if l2_28 else [])))):
            what = "%s msd2=%d work=%d (levels %d / %d / %d)" % (key, msd2, wb, l0, l2, l1)
            status, labels, _ = run.run(i, wb, fill="random" if i % 3 == 2 else "ff", what=what)
            assert status == "sorted"
            forms.append((wb, _form(labels)))
        SWEEP_FORMS["%s-msd2=%d" % (key, msd2)] = forms
        names = [f for _, f in forms]
        assert len(set(names)) >= 2, (key, msd2, forms)                      # the sweep must not stay on one path
        assert names[0] == "threekernel", (key, msd2, forms)                  # level 0: the reference's own contract
        large = [f.startswith("large") for f in names]
        assert large[-1], (key, msd2, forms)                                  # level 1: the large sort
        first = large.index(True)
        assert all(large[first:]), (key, msd2, forms)                         # more work never leaves the large sort
        at_l2 = [f for wb, f in forms if wb == l2][0]
        assert at_l2.startswith("large"), (key, msd2, forms)                  # level 2 keeps the large sort
        if l2_28:
            at = [f for wb, f in forms if wb == l2_28][0]
            assert at.startswith("large"), ("a 28-bit sort's lean work - 1", key, msd2, forms)
    _dump_report()


def _dump_report():
    path = os.environ.get("ADLHIP_CONTRACT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"sweep_forms": SWEEP_FORMS, "labels": sorted(SEEN_LABELS), "net": sorted(NET_FAMILIES)}, f, indent=1)


def _edges_below(esz):
    return sorted({(8 * Mi) // esz, (24 * Mi) // esz - 1, 16 * Mi - 1, 2 * Mi - 1, 2 * Mi + 1, Mi - 1, Mi + 1, 16385})


@pytest.mark.parametrize("kind", [U32, KV32, U64, SOA32], ids=["u32", "kv32", "u64", "soa32"])
def test_scratch_sized_once_for_the_largest_batch(dev, arena, kind):
    """adlhip_radix_sort_scratch_bytes(N) for N = 20 Mi + 77 suffices for every smaller n' at the edges sort_work_bytes lists; the
    same guarded tmp / work regions serve every n'.  Then the knobs change after sizing (256 x 16 tiles, 4-bit digits, one-sweep
    passes): every call sorts exactly or is refused without touching memory."""
    N = 20 * Mi + 77
    tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    check(_lib.load().adlhip_radix_sort_scratch_bytes(dev._h, kind, N, ctypes.byref(tb), ctypes.byref(wb)), "scratch_bytes")
    work = wb.value
    bits = MAX_BITS[kind]
    for i, n in enumerate(_edges_below(ESZ[kind])):
        assert n < N
        run = SortRun(dev, arena, 200 + i, kind, n, "uniform", bits, tmp_n=N)
        status, _, _ = run.run(200 + i, work, fill="random" if i % 3 == 1 else "ff", what="%s n'=%d in scratch for %d" % (KIND_NAME[kind], n, N))
        assert status == "sorted"
    set_knobs(dev, {"sort.tile": 0, "sort.digit_bits": 4, "sort.algo": 0})
    outcomes = []
    for i, n in enumerate([N, 2 * Mi + 1, 16385]):
        run = SortRun(dev, arena, 300 + i, kind, n, "uniform", bits, tmp_n=N)
        status, _, _ = run.run(300 + i, work, what="%s n'=%d after the knobs changed" % (KIND_NAME[kind], n), expect_refusal=None)
        outcomes.append((n, status))
    assert any(s == "sorted" for _, s in outcomes), outcomes


# ---------------------------------------------------------------------------------------------
# refused calls leave everything untouched
# ---------------------------------------------------------------------------------------------
def _refusal(dev, arena, case_no, kind, n, bits, work_bytes, shift=None, call=None, knobs=None):
    set_knobs(dev, knobs or {})
    esz = ESZ[kind]
    L = Layout(arena, case_no)
    poison = U32 if esz == 4 else (KV32 if kind == KV32 else U64)
    regs = {"data": L.add("data", n * esz, poison=poison, shift=shift.get("data") if shift else None)}
    if kind == SOA32:
        regs["vals"] = L.add("vals", n * 4, poison="u32v", shift=shift.get("vals") if shift else None)
    regs["tmp"] = L.add("tmp", n * esz)
    if kind == SOA32:
        regs["tmpv"] = L.add("tmp_vals", n * 4)
    regs["work"] = L.add("work", work_bytes, shift=shift.get("work") if shift else None)
    L.commit()
    L.upload(regs["data"], make_keys(64 if kind == U64 else 32, n * (2 if kind == KV32 else 1), "uniform", case_no).view(
        np.uint64 if kind in (KV32, U64) else np.uint32))
    L.prefill(regs["tmp"], "random")
    L.prefill(regs["work"], "ff")
    sync(dev)
    before = L.snapshot()
    rc, labels, _ = run_profiled(dev, (lambda: call(regs)) if call else (lambda: sort_call(dev, kind, regs, work_bytes, n, bits)))
    err = _lib_err()
    assert rc != 0, "call was not refused"
    assert err, "refused without an error text"
    rc_sync = _lib.load().adlhip_sync(dev._h)
    assert rc_sync == 0, "fault word set by a refused call: %s" % _lib_err()
    assert not labels, labels
    after = L.snapshot()
    if not np.array_equal(after, before):
        diff = np.flatnonzero(after != before)
        raise AssertionError("a refused call changed %d bytes of the arena, first at %d" % (diff.size, diff[0]))
    return err


REFUSALS = ["work-level0-minus-1", "data-at-plus-4", "work-at-plus-4", "tmp-at-plus-8", "sort-bits-30", "n-beyond-kMaxElems",
            "onesweep-work-too-small"]


@pytest.mark.parametrize("kind", [U32, KV32, U64, SOA32], ids=["u32", "kv32", "u64", "soa32"])
@pytest.mark.parametrize("what", REFUSALS)
def test_refused_calls_leave_memory_untouched(dev, arena, what, kind):
    n = 3 * Mi + 17 if kind in (U32, SOA32) else Mi + 1
    bits = MAX_BITS[kind]
    l0 = scratch_for(dev, kind, n, bits, 0)[1]
    l1 = scratch_for(dev, kind, n, bits, 1)[1]
    case_no = 400 + REFUSALS.index(what) * 4 + kind
    if what == "work-level0-minus-1":
        _refusal(dev, arena, case_no, kind, n, bits, l0 - 1)
    elif what == "data-at-plus-4":
        _refusal(dev, arena, case_no, kind, n, bits, l1, shift={"data": 4})
    elif what == "work-at-plus-4":
        _refusal(dev, arena, case_no, kind, n, bits, l1, shift={"work": 4})
    elif what == "tmp-at-plus-8":
        def call(regs):
            tmp = ctypes.c_void_p(regs["tmp"].addr + 8)
            lib, h = _lib.load(), dev._h
            fn = {U32: lib.adlhip_radix_sort_u32, KV32: lib.adlhip_radix_sort_kv32, U64: lib.adlhip_radix_sort_u64}.get(kind)
            if fn is None:
                return lib.adlhip_radix_sort_soa32(h, regs["data"].ptr, regs["vals"].ptr, tmp, regs["tmpv"].ptr, regs["work"].ptr, l1, n - 2, bits)
            return fn(h, regs["data"].ptr, tmp, regs["work"].ptr, l1, n - 2, bits)
        _refusal(dev, arena, case_no, kind, n, bits, l1, call=call)
    elif what == "sort-bits-30":
        _refusal(dev, arena, case_no, kind, n, 30, l1)
    elif what == "n-beyond-kMaxElems":
        def call(regs):
            return sort_call(dev, kind, regs, l1, K_MAX_ELEMS + 1, bits)
        _refusal(dev, arena, case_no, kind, 4097, bits, l1, call=call)
    else:       # work sized by the reference's contract for the default knobs, then one-sweep passes on small tiles and 4-bit digits
        _refusal(dev, arena, case_no, kind, n, bits, l0, knobs={"sort.tile": 0, "sort.digit_bits": 4, "sort.algo": 0})


# ---------------------------------------------------------------------------------------------
# the other primitives, in the same arena
# ---------------------------------------------------------------------------------------------
SCAN_SIZES = [1, 3, 4095, 4096, 4097, 65537, Mi + 1, 6 * Mi + 3, 64 * Mi + 5]


@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "inplace"])
def test_exclusive_scan_stays_inside_its_buffers(dev, arena, inplace):
    lib = _lib.load()
    for i, n in enumerate(SCAN_SIZES):
        rng = np.random.default_rng(n)
        src = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if i % 2 else rng.integers(0, 64, n, dtype=np.uint32)
        want, total = oracle.exclusive_scan_u32(src)
        wb = ctypes.c_size_t()
        check(lib.adlhip_scan_scratch_bytes(dev._h, n, ctypes.byref(wb)), "scan_scratch_bytes")
        L = Layout(arena, 500 + i + (50 if inplace else 0))
        rs = L.add("src", 4 * n, poison=U32)
        rd = rs if inplace else L.add("dst", 4 * n, poison=U32)
        rw = L.add("work", wb.value)
        L.commit()
        L.upload(rs, src)
        if not inplace:
            L.prefill(rd, "random")
        L.prefill(rw, "ff" if i % 3 else "random")
        h_total = np.full(1, 0xDEADBEEF, dtype=np.uint32)
        rc, _, _ = run_profiled(dev, lambda: lib.adlhip_exclusive_scan_u32(dev._h, rd.ptr, rs.ptr, rw.ptr, wb.value, n,
                                                                         h_total.ctypes.data_as(ctypes.c_void_p)))
        assert rc == 0, _lib_err()
        sync(dev)
        assert np.array_equal(L.fetch(rd, np.uint32), want), (n, inplace)
        assert int(h_total[0]) == total, (n, int(h_total[0]), total)
        if not inplace:
            assert np.array_equal(L.fetch(rs, np.uint32), src), "scan changed its source (n=%d)" % n
        L.assert_bands_intact("scan n=%d inplace=%s" % (n, inplace))


def _partition_expected(arr, keys, shift):
    """(expected output, bucket of every key) of a partition by the keys' bits from `shift` up: stable by the top byte (which
    refines the buckets without mixing them, adlhip.hip partition_msb); one bucket is a plain copy."""
    bucket = (keys.astype(np.uint64) >> np.uint64(shift)) if shift < 32 else np.zeros(keys.size, np.uint64)
    if shift >= 32:
        return arr.copy(), bucket
    top = keys.astype(np.uint64) >> np.uint64(24)
    order = (np.sort((top << np.uint64(32)) | np.arange(keys.size, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return arr[order], bucket


@pytest.mark.parametrize("kind", [U32, KV32], ids=["u32", "kv32"])
def test_partition_msb_stays_inside_its_buffers(dev, arena, kind):
    lib = _lib.load()
    fn = lib.adlhip_partition_msb_u32 if kind == U32 else lib.adlhip_partition_msb_kv32
    esz = ESZ[kind]
    case = 600 + 100 * kind
    for n in (1, 4097, 6 * Mi + 3, 8 * Mi + 1):
        keys = make_keys(32, n, "heavy" if n > 4097 else "uniform", n)
        arr = keys if kind == U32 else keys.astype(np.uint64) | (np.arange(n, dtype=np.uint64) << np.uint64(32))
        levels = {0: scratch_for(dev, kind, n, 32, 0)[1], 1: scratch_for(dev, kind, n, 32, 1)[1]}
        for j, buckets in enumerate((1, 2, 16, 256)):
            lg = buckets.bit_length() - 1
            for level in ((0, 1) if n <= 4097 else (j % 2,)):
                # level 1 from 24 MiB of data: the look-back variant, and (last) the same call with the knob off
                set_knobs(dev, {"partition.lookback": 0 if j == 3 else 1})
                wb = levels[level]
                case += 1
                L = Layout(arena, case)
                rin = L.add("in", n * esz, poison=kind)
                rout = L.add("out", n * esz, poison=kind)
                rc_ = L.add("counts", 4 * buckets)
                rw = L.add("work", wb)
                L.commit()
                L.upload(rin, arr)
                L.prefill(rout, "random")
                L.prefill(rc_, "ff")
                L.prefill(rw, "ff" if case % 3 else "random")
                rc, _, _ = run_profiled(dev, lambda: fn(dev._h, rin.ptr, rout.ptr, rc_.ptr, rw.ptr, wb, n, buckets))
                assert rc == 0, _lib_err()
                sync(dev)
                want, bucket = _partition_expected(arr, keys, 32 - lg)
                what = "partition %s n=%d buckets=%d level=%d" % (KIND_NAME[kind], n, buckets, level)
                assert np.array_equal(L.fetch(rout, arr.dtype), want), what
                assert np.array_equal(L.fetch(rc_, np.uint32), np.bincount(bucket.astype(np.int64), minlength=buckets).astype(np.uint32)), what
                assert np.array_equal(L.fetch(rin, arr.dtype), arr), what + ": input changed"
                L.assert_bands_intact(what)


@pytest.mark.parametrize("kind", [U32, KV32], ids=["u32", "kv32"])
def test_partition_refuses_an_unaligned_work_buffer(dev, arena, kind):
    """Work at +4 bytes: refused with an error text, nothing enqueued, the arena byte-identical, the fault word clear."""
    lib = _lib.load()
    n, esz = 6 * Mi + 3, ESZ[kind]
    wb = scratch_for(dev, kind, n, 32, 1)[1]
    L = Layout(arena, 700 + kind)
    rin = L.add("in", n * esz, poison=kind)
    rout = L.add("out", n * esz, poison=kind)
    rc_ = L.add("counts", 4 * 256)
    rw = L.add("work", wb, shift=4)
    L.commit()
    L.upload(rin, make_keys(32, n * (esz // 4), "uniform", 7).view(np.uint32 if kind == U32 else np.uint64))
    L.prefill(rw, "ff")
    sync(dev)
    before = L.snapshot()
    for fn, args in ((lib.adlhip_partition_msb_u32 if kind == U32 else lib.adlhip_partition_msb_kv32, (16,)),
                     (lib.adlhip_partition_top_byte_u32 if kind == U32 else lib.adlhip_partition_top_byte_kv32, ())):
        rc, labels, _ = run_profiled(dev, lambda: fn(dev._h, rin.ptr, rout.ptr, rc_.ptr, rw.ptr, wb, n, *args))
        assert rc != 0 and _lib_err(), "an unaligned work buffer was accepted"
        assert not labels, labels
        assert _lib.load().adlhip_sync(dev._h) == 0, _lib_err()
    assert np.array_equal(L.snapshot(), before), "a refused partition changed memory"


@pytest.mark.parametrize("kind", [U32, KV32], ids=["u32", "kv32"])
def test_partition_top_byte_stays_inside_its_buffers(dev, arena, kind):
    lib = _lib.load()
    fn = lib.adlhip_partition_top_byte_u32 if kind == U32 else lib.adlhip_partition_top_byte_kv32
    esz = ESZ[kind]
    for i, (n, level) in enumerate(((4097, 0), (Mi + 1, 1), (6 * Mi + 3, 1), (6 * Mi + 3, 0), (8 * Mi + 1, 1))):
        keys = make_keys(32, n, "uniform" if i % 2 else "few256", n + kind)
        arr = keys if kind == U32 else keys.astype(np.uint64) | (np.arange(n, dtype=np.uint64) << np.uint64(32))
        wb = scratch_for(dev, kind, n, 32, level)[1]
        L = Layout(arena, 800 + i + 10 * kind)
        rin = L.add("in", n * esz, poison=kind)
        rout = L.add("out", n * esz, poison=kind)
        rt = L.add("totals256", 256 * 4)
        rw = L.add("work", wb)
        L.commit()
        L.upload(rin, arr)
        L.prefill(rout, "random")
        L.prefill(rt, "ff")
        L.prefill(rw, "ff" if i % 3 else "random")
        rc, _, _ = run_profiled(dev, lambda: fn(dev._h, rin.ptr, rout.ptr, rt.ptr, rw.ptr, wb, n))
        assert rc == 0, _lib_err()
        sync(dev)
        want, bucket = _partition_expected(arr, keys, 24)
        what = "top-byte partition %s n=%d level=%d" % (KIND_NAME[kind], n, level)
        assert np.array_equal(L.fetch(rout, arr.dtype), want), what
        assert np.array_equal(L.fetch(rt, np.uint32), np.bincount(bucket.astype(np.int64), minlength=256).astype(np.uint32)), what
        assert np.array_equal(L.fetch(rin, arr.dtype), arr), what + ": input changed"
        L.assert_bands_intact(what)


@pytest.mark.parametrize("kind", [U32, KV32], ids=["u32", "kv32"])
@pytest.mark.parametrize("low_bits", [8, 24, 27])
def test_segment_sort_leaves_the_rest_of_the_array_alone(dev, arena, kind, low_bits):
    lib = _lib.load()
    bound = (16384 if kind == U32 else 8192) // (2 if low_bits > 24 else 1)
    rng = np.random.default_rng(low_bits * 10 + kind)
    sizes = np.concatenate([[0, bound, 1, 0, 0], rng.integers(0, bound + 1, 40), [bound - 1, 0, bound]]).astype(np.int64)
    lo = 1237                                    # the segments cover [lo, hi) of a larger array
    starts = (lo + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint32)
    hi = int(starts[-1])
    total = hi + 3001
    keys = oracle.keys_u32(total, seed=low_bits + 17 * kind)
    arr = keys if kind == U32 else keys.astype(np.uint64) | (np.arange(total, dtype=np.uint64) << np.uint64(32))
    L = Layout(arena, 900 + low_bits + kind)
    rd = L.add("data", arr.nbytes, poison=kind)
    rs = L.add("seg_start", starts.nbytes)
    L.commit()
    L.upload(rd, arr)
    L.upload(rs, starts)
    rc, _, _ = run_profiled(dev, lambda: lib.adlhip_segment_sort(dev._h, kind, rd.ptr, rs.ptr, starts.size - 1, bound, low_bits))
    assert rc == 0, _lib_err()
    sync(dev)
    got = L.fetch(rd, arr.dtype)
    want = arr.copy()
    seg = arr[lo:hi]
    seg_id = np.repeat(np.arange(sizes.size, dtype=np.uint64), sizes)
    low = seg.astype(np.uint64) & np.uint64((1 << low_bits) - 1)
    want[lo:hi] = seg[np.argsort((seg_id << np.uint64(32)) | low, kind="stable")]
    assert np.array_equal(got[:lo], arr[:lo]) and np.array_equal(got[hi:], arr[hi:]), "elements outside the segments changed"
    assert np.array_equal(got, want)
    assert np.array_equal(L.fetch(rs, np.uint32), starts)
    L.assert_bands_intact("segment sort %s low_bits=%d" % (KIND_NAME[kind], low_bits))


FILL_COUNTS = [1, 3, 5, 4097, Mi + 3]


@pytest.mark.parametrize("op", ["fill_u32", "fill_pattern4", "fill_pattern8", "fill_pattern16", "memset", "memcpy_d2d"])
def test_fill_and_copy_write_exactly_their_bytes(dev, arena, op):
    lib = _lib.load()
    elem = {"fill_u32": 4, "fill_pattern4": 4, "fill_pattern8": 8, "fill_pattern16": 16, "memset": 1, "memcpy_d2d": 1}[op]
    for i, count in enumerate(FILL_COUNTS):
        for minimal in (False, True):
            shift = (elem if elem < 16 else 16) if minimal else 0
            if op in ("memset", "memcpy_d2d") and minimal:
                shift = 1 + 2 * (i % 3)         # byte-aligned destinations
            L = Layout(arena, 1000 + i * 2 + minimal)
            nbytes = count * elem
            rd = L.add("dst", nbytes, shift=shift)
            rs = L.add("src", nbytes, shift=3 if minimal else 0) if op == "memcpy_d2d" else None
            L.commit()
            L.prefill(rd, "random")
            pat = np.frombuffer(np.random.default_rng(count + elem).bytes(max(elem, 4)), dtype=np.uint8)[:elem]
            if op == "memcpy_d2d":
                src = np.frombuffer(np.random.default_rng(count).bytes(nbytes), dtype=np.uint8)
                L.upload(rs, src)
                want = src
                fn = lambda: lib.adlhip_memcpy_d2d(dev._h, rd.ptr, rs.ptr, nbytes)
            elif op == "memset":
                want = np.full(nbytes, 0xA5, dtype=np.uint8)
                fn = lambda: lib.adlhip_memset(dev._h, rd.ptr, 0xA5, nbytes)
            elif op == "fill_u32":
                v = int(pat.view(np.uint32)[0])
                want = np.full(count, v, dtype=np.uint32).view(np.uint8)
                fn = lambda: lib.adlhip_fill_u32(dev._h, rd.ptr, v, count)
            else:
                want = np.tile(pat, count)
                fn = lambda: lib.adlhip_fill_pattern(dev._h, rd.ptr, pat.ctypes.data_as(ctypes.c_void_p), elem, count)
            sync(dev)
            rc, _, _ = run_profiled(dev, fn)
            assert rc == 0, _lib_err()
            sync(dev)
            what = "%s count=%d at %d (mod 256)" % (op, count, rd.off % 256)
            assert np.array_equal(L.fetch(rd, np.uint8), want), what
            if rs is not None:
                assert np.array_equal(L.fetch(rs, np.uint8), src), what + ": source changed"
            L.assert_bands_intact(what)


@pytest.mark.parametrize("kind", [U32, KV32, U64], ids=["u32", "kv32", "u64"])
def test_generate_keys_writes_exactly_n_elements(dev, arena, kind):
    lib = _lib.load()
    for i, n in enumerate((1, 4097, Mi + 3)):
        esz = ESZ[kind]
        L = Layout(arena, 1100 + 3 * kind + i)
        rd = L.add("data", n * esz, poison=kind)
        L.commit()
        L.prefill(rd, "random")
        rc, _, _ = run_profiled(dev, lambda: lib.adlhip_generate_keys(dev._h, kind, rd.ptr, n, 99, 77))
        assert rc == 0, _lib_err()
        sync(dev)
        want = {U32: oracle.keys_u32, KV32: oracle.pairs_kv32, U64: oracle.keys_u64}[kind](n, seed=99, first_index=77)
        assert np.array_equal(L.fetch(rd, want.dtype), want), (kind, n)
        L.assert_bands_intact("generate_keys kind=%d n=%d" % (kind, n))


# ---------------------------------------------------------------------------------------------
# SoA sorts of wide keys / values
# ---------------------------------------------------------------------------------------------
SOA_WIDE = [(4, 8, 32), (8, 4, 44), (8, 16, 64)]


@pytest.mark.parametrize("widths", SOA_WIDE, ids=["k32-v64-tmpkeysNULL", "k64-v32-44bits", "k64-v128"])
@pytest.mark.parametrize("n", [70001, 3 * Mi + 17])
def test_soa_wide_sort_stays_inside_its_buffers(dev, arena, widths, n):
    lib = _lib.load()
    kb, vb, bits = widths
    tk, tv, wbv = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.adlhip_radix_sort_soa_scratch_bytes(dev._h, kb, vb, n, bits, ctypes.byref(tk), ctypes.byref(tv), ctypes.byref(wbv)), "soa scratch")
    keys = make_keys(8 * kb, n, "few256" if n < Mi else "uniform", n + kb)
    idx = np.arange(n, dtype=np.uint64)
    if vb == 4:
        vals = idx.astype(np.uint32)
    elif vb == 8:
        vals = idx | np.uint64(MARKER << 32)
    else:
        vals = np.stack([idx.astype(np.uint32), ~idx.astype(np.uint32), np.full(n, MARKER, np.uint32), (idx * 3).astype(np.uint32)], axis=1)
    case = 1200 + n % 7 + kb + vb
    L = Layout(arena, case)
    rk = L.add("keys", n * kb, poison=U32 if kb == 4 else U64)
    rv = L.add("vals", n * vb, poison="u32v")
    rtk = L.add("tmp_keys", n * kb) if kb == 8 else None
    rtv = L.add("tmp_vals", n * vb)
    rw = L.add("work", wbv.value)
    L.commit()
    L.upload(rk, keys)
    L.upload(rv, vals)
    for r in (rtk, rtv, rw):
        if r is not None:
            L.prefill(r, "ff" if case % 3 else "random")
    rc, labels, _ = run_profiled(dev, lambda: lib.adlhip_radix_sort_soa(dev._h, rk.ptr, kb, rv.ptr, vb, rtk.ptr if rtk else None, rtv.ptr, rw.ptr,
                                                                      wbv.value, n, bits))
    assert rc == 0, _lib_err()
    sync(dev)
    order = stable_order(keys, bits)
    what = "soa k%d v%d bits %d n=%d" % (kb, vb, bits, n)
    assert np.array_equal(L.fetch(rk, keys.dtype), keys[order]), what
    gv = L.fetch(rv, np.uint32).reshape(n, -1) if vb == 16 else L.fetch(rv, vals.dtype)
    assert np.array_equal(gv, vals[order]), what
    L.assert_bands_intact(what)


# ---------------------------------------------------------------------------------------------
# positive control and coverage (last: coverage is the union over the module)
# ---------------------------------------------------------------------------------------------
def test_guard_check_sees_a_three_word_overrun(dev, arena):
    """Sorting n + 3 keys in a region declared as n elements writes the first three words of the poison band after it: the
    checker must report exactly those 12 bytes and nothing else in the arena.  (It writes only inside the test's allocation.)"""
    n = 4097
    keys = make_keys(32, n, "uniform", 5)
    tb, wb = scratch_for(dev, U32, n + 3, 32, 1)
    L = Layout(arena, 1301)
    rd = L.add("data", 4 * n, poison=U32)
    rt = L.add("tmp", 4 * (n + 3))
    rw = L.add("work", wb)
    L.commit()
    L.upload(rd, keys)
    L.prefill(rt, "ff")
    L.prefill(rw, "ff")
    rc, _, _ = run_profiled(dev, lambda: _lib.load().adlhip_radix_sort_u32(dev._h, rd.ptr, rt.ptr, rw.ptr, wb, n + 3, 32))
    assert rc == 0, _lib_err()
    sync(dev)
    bad = L.band_damage()
    assert len(bad) == 1, bad
    name, side, first, last, count, _, _ = bad[0]
    assert (name, side) == ("data", "after"), bad
    assert 4 * n <= first <= last < 4 * n + 12, bad
    # and the sorted n + 3 keys are the input with the poison's 0, ~0, 0 folded in
    full = L.read(rd.off, 4 * (n + 3), np.uint32)
    sync(dev)
    assert np.array_equal(full, np.sort(np.concatenate([keys, np.array([0, 0xFFFFFFFF, 0], np.uint32)])))


# family -> alternatives: the family is reached when every label of one alternative was seen
PATH_FAMILIES = {
    "one-workgroup small sort": [{"small_sort_u32"}, {"small_sort_e64"}],
    "mid-size sort, two launches": [{"mid_bucket_scatter_u32", "segment_sort_u32"}],
    "mid-size sort, three launches": [{"mid_prep_u32", "onesweep_u32_8b", "segment_sort_u32"}],
    "three-kernel passes": [{"count_u32_8b", "scan_table", "scatter_u32_8b"}],
    "one-sweep passes": [{"os_hist_u32", "os_hist_reduce", "os_tables", "onesweep_u32_4b"}],
    "LARGE_U32": [{"msd2_sample", "msd2_pass1_u32", "msd2_pass2_u32", "msd2_offsets", "segment_sort_wave_u32"}],
    "workgroup-per-segment finish": [{"segment_sort_wg_u32"}],
    "LARGE_PAIRS": [{"msd2s_prep", "msd2s_pass1_kv32", "msd2s_pass2_kv32", "msd2s_offsets", "segment_sort_wave_e64"}],
    "LARGE_U64_BIN": [{"msd2s_prep", "msd2s_pass1_u64", "msd2s_pass2_u64", "msd2s_offsets", "segment_sort_bin_u64", "segment_sort_listed_e64"}],
    "LARGE_U64_LSD": [{"msd2s_prep", "msd2s_pass1_u64", "msd2s_pass2_u64", "msd2s_offsets", "segment_sort_wave_e64"}],
    "large sort of SoA pairs": [{"msd2s_pass1_soa", "msd2s_pass2_soa"}],
    "soa_gather": [{"soa_pack_index_k32", "soa_pack_index_k64", "soa_gather"}],
    "soa_repack_high": [{"soa_repack_high"}],
    "scan": [{"scan_single", "scan_reduce", "scan_partials", "scan_apply"}],
    "partition": [{"fold_buckets", "count_u32_8b", "scatter_u32_8b"}, {"fold_buckets", "onesweep_u32_8b"}],
    "fill": [{"fill_u32", "fill_pattern"}],
    "generate": [{"generate_keys"}],
}
NET_FAMILY_NAMES = {"net_counting", "net_counting_dict4096", "net_lsd_lookback", "net_lsd_count_scan_scatter"}


def test_the_module_reached_every_path_family():
    """The union of the kernels the module ran covers every path family, and the large sort's safety net ran by counting (both
    dictionaries) and by LSD passes (look-back and count-scan-scatter).  If the matrix stops reaching a family, this fails."""
    _dump_report()
    missing = {fam: [sorted(a - SEEN_LABELS) for a in alts] for fam, alts in PATH_FAMILIES.items() if not any(a <= SEEN_LABELS for a in alts)}
    assert not missing, "path families not reached: %s (seen: %s)" % (missing, sorted(SEEN_LABELS))
    assert NET_FAMILY_NAMES <= NET_FAMILIES, "safety-net families not reached: %s" % sorted(NET_FAMILY_NAMES - NET_FAMILIES)
