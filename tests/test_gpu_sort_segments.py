"""Sort and argsort within variable-length segments on the GPU (include/adlhip.h adlhip_sort_segments_typed;
oclradixsort_amd/csrc/segments_kernels.hpp; Pprims.sortSegments; TorchSorter.sort_segments / argsort_segments).

The expected output is independent of the code under test: the keys are encoded with the numpy codec of tests/typed_shapes.py
(encoded_dwords: a key's ordinal moved into the unsigned range; descending: its complement) and every segment's expectation is
np.argsort(codes_of_the_segment, kind="stable").  Indices and key bits must be equal; there is no tolerance anywhere.

Every call of run() checks the whole memory contract: both outputs and the count word lie between guard regions that are unchanged
afterwards, the input (which starts 48 bytes into its allocation) and the offsets are unchanged, the work buffer has exactly the
reported size, holds garbage on entry and has guards of its own, adlhip_fault_check is clean and the handle's device state is idle
(the check of test_gpu_call_sequences.py).  Every case runs keys only, indices only and both.  Calls of different shapes follow each
other on one handle throughout.

G_k below is the number of listed segments a tile of class k takes: 4096 >> k, class k holding the lengths in (2^(k-1), 2^k] (and 1
for k = 1).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

from oclradixsort_amd import Buffer, DeviceUtils, _lib
from test_gpu_call_sequences import assert_idle
from typed_shapes import ASC, BY_NAME, DESC, SPECIALS, encoded_dwords, shape

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "sort_segments_demo")
TYPE_IDS = ["u32", "i32", "f32", "u64", "i64", "f64"]
CAP = 4096
KERNEL, FLAT, AUTO = 1, 0, -1
LOCAL, GLOBAL = 0, 1
BOTH, KEYS_ONLY, INDEX_ONLY = "both", "keys", "index"
MODES = (BOTH, KEYS_ONLY, INDEX_ONLY)


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


def expected_segments(bits, name, offsets, order):
    """(local indices int64 [n], key bits [n]) of the stable argsort of every segment"""
    codes = codes_of(bits, name, order)
    idx = np.zeros(bits.size, np.int64)
    for s in range(len(offsets) - 1):
        a, b = int(offsets[s]), int(offsets[s + 1])
        if b > a:
            idx[a:b] = np.argsort(codes[a:b], kind="stable")
    starts = np.repeat(np.asarray(offsets[:-1], np.int64), np.diff(np.asarray(offsets, np.int64)))
    return idx, bits[idx + starts]


def random_bits(udt, n, seed, specials=True):
    rng = np.random.default_rng(seed)
    w = np.dtype(udt).itemsize
    x = np.frombuffer(rng.bytes(w * max(n, 1)), dtype=udt)[:n].copy()
    if specials and n >= 8:   # +-NaN of several payloads, +-0, +-inf, denormals, the extremes of the integer readings
        sp = SPECIALS[w]
        at = rng.choice(n, size=min(n // 2, 3 * sp.size), replace=False)
        x[at] = np.resize(sp, at.size)
    return x


def class_edge_lengths():
    """0, 1, 2, 3, 2^k - 1, 2^k, 2^k + 1 for k = 2 .. 11, 4095 and 4096, shuffled; empty segments first, last and in a run"""
    core = [0, 1, 2, 3, 4095, 4096]
    for k in range(2, 12):
        core += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    rng = np.random.default_rng(2024)
    core = [int(x) for x in rng.permutation(core)]
    lens = [0, 0] + core[:11] + [0, 0, 0] + core[11:] + [0]
    classes = set(0 if x == 0 else max(1, int(np.ceil(np.log2(x)))) for x in lens)
    assert classes == set(range(13)) and lens[0] == 0 and lens[-1] == 0
    return lens


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
def lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


def reset(d):
    d.setParam("sort.segments_algo", -1)
    d.setParam("debug.sort_segments_grid", 0)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    reset(d)
    DeviceUtils.deallocate(d)


class Framed:
    """nbytes of payload on the device between two guard regions; the payload starts `front` bytes (a multiple of 16) into the
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
        """the payload; asserts that the guards are what they were"""
        raw = self.buf.toHost()
        a, b = self.front, self.front + self.nbytes
        assert np.array_equal(raw[:a], self.image[:a]), "bytes in front of the buffer were written"
        assert np.array_equal(raw[b:], self.image[b:]), "bytes behind the buffer were written"
        return raw[a:b].view(dtype)

    def unchanged(self):
        return np.array_equal(self.read(), self.image[self.front:self.front + self.nbytes])

    def release(self):
        self.buf.release()


def scratch_bytes(dev, kt, n, S, bound):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_sort_segments_scratch_bytes(dev._h, kt, n, S, bound, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


class Case:
    """n keys in segments on the device and every order's expectation (computed once)"""

    def __init__(self, dev, name, bits, lens, device_offsets=None):
        self.dev, self.name, self.kt, self.udt = dev, name, BY_NAME[name][1], BY_NAME[name][3]
        self.lens = [int(x) for x in lens]
        self.offsets = offsets_of(self.lens)
        self.n, self.S = int(self.offsets[-1]), len(self.lens)
        assert bits.dtype == self.udt and bits.size == self.n
        self.bits = bits
        self.inp = Framed(dev, payload=bits if bits.size else np.zeros(2, self.udt), front=48, seed=5)   # 48: an odd multiple of 16 bytes
        self.off = Framed(dev, payload=self.offsets if device_offsets is None else np.asarray(device_offsets, np.uint32), seed=9)
        self.checked = device_offsets is None   # offsets that break the contract: only the memory contract is checked
        self._want = {}

    def expected(self, order):
        if order not in self._want:
            self._want[order] = expected_segments(self.bits, self.name, self.offsets, order)
        return self._want[order]

    def run(self, order, mode=BOTH, base=LOCAL, bound=None, want_oversized=0, passthrough=()):
        """one call under the knobs in force; returns (index bytes or None, key bytes or None) after every check.  bound: max_segment
        (default: the longest segment).  passthrough: the segments expected in input order with identity indices."""
        w_item = self.bits.dtype.itemsize
        n, S = self.n, self.S
        bound = max(self.lens) if bound is None else bound
        need = scratch_bytes(self.dev, self.kt, n, S, bound)
        ko = Framed(self.dev, nbytes=max(n, 1) * w_item, seed=6) if mode != INDEX_ONLY else None
        io = Framed(self.dev, nbytes=max(n, 1) * 4, seed=7) if mode != KEYS_ONLY else None
        cw = Framed(self.dev, nbytes=16, fill=0x5c, seed=10)   # the count word is its bytes 4 .. 7
        work = Framed(self.dev, nbytes=max(need, 16), fill=0xa7, seed=8)   # garbage on entry
        try:
            rc = _lib.load().adlhip_sort_segments_typed(self.dev._h, self.kt, order, self.inp.ptr(), n, self.off.ptr(), S, bound, base,
                                                        ko.ptr() if ko else None, io.ptr() if io else None, cw.ptr(4), work.ptr(), need)
            assert rc == 0, lib_err()
            got_i = io.read(np.uint32)[:n] if io else None
            got_k = ko.read(self.udt)[:n] if ko else None
            work.read()   # (checks the guards of the work buffer)
            word = cw.read(np.uint32)
            assert word[0] == 0x5c5c5c5c and word[2] == 0x5c5c5c5c and word[3] == 0x5c5c5c5c, "bytes beside the count word were written"
            assert self.inp.unchanged(), "the sort changed d_keys_in"
            assert self.off.unchanged(), "the sort changed d_offsets"
            self.dev.checkFault()
            assert_idle(self.dev, "sort of segments")
            if not self.checked:
                return None
            assert int(word[1]) == want_oversized, "the count word is %d, expected %d" % (int(word[1]), want_oversized)
            want_i, want_k = self.expected(order)
            want_i, want_k = want_i.copy(), want_k.copy()
            for s in passthrough:
                a, b = int(self.offsets[s]), int(self.offsets[s + 1])
                want_i[a:b] = np.arange(b - a)
                want_k[a:b] = self.bits[a:b]
            if base == GLOBAL:
                want_i = want_i + np.repeat(self.offsets[:-1].astype(np.int64), np.diff(self.offsets.astype(np.int64)))
            what = "%s order %d S %d n %d base %d bound %d %s" % (self.name, order, S, n, base, bound, mode)
            seg_of = np.repeat(np.arange(S), np.diff(self.offsets.astype(np.int64)))
            if io:
                bad = np.unique(seg_of[got_i.astype(np.int64) != want_i])
                assert bad.size == 0, "%s: indices differ in segments %s (lengths %s)" % (what, bad[:8].tolist(), [self.lens[s] for s in bad[:8]])
            if ko:
                bad = np.unique(seg_of[got_k != want_k])
                assert bad.size == 0, "%s: keys differ in segments %s (lengths %s)" % (what, bad[:8].tolist(), [self.lens[s] for s in bad[:8]])
            return (got_i.tobytes() if io else None, got_k.tobytes() if ko else None)
        finally:
            for b in (ko, io, cw, work):
                if b is not None:
                    b.release()

    def run_modes(self, order, base=LOCAL, **kw):
        """keys only, indices only and both"""
        return [self.run(order, mode, base, **kw) for mode in MODES]

    def release(self):
        self.inp.release()
        self.off.release()


def make_case(dev, name, lens, seed=0, bits=None):
    n = int(sum(lens))
    udt = BY_NAME[name][3]
    flat = random_bits(udt, n, seed) if bits is None else bits(n)
    return Case(dev, name, np.ascontiguousarray(flat, dtype=udt), lens)


@pytest.fixture(scope="module")
def edge_cases(dev):
    """the class-edge call for every key type: built once, shared, never changed"""
    lens = class_edge_lengths()
    cases = {name: make_case(dev, name, lens, seed=17 + i) for i, name in enumerate(TYPE_IDS)}
    yield cases
    for c in cases.values():
        c.release()


# ---------------------------------------------------------------------------------------------
# 1. class edges: every class in one call, every type, both orders, both index bases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TYPE_IDS)
def test_class_edges_every_type_order_and_index_base(dev, edge_cases, name):
    c = edge_cases[name]
    assert np.isin(SPECIALS[c.bits.dtype.itemsize], c.bits).all()
    assert dev.getParam("sort.segments_algo") == AUTO   # (a bound of 4096: the segment kernel, see test_scratch_query_matches_its_formula)
    for order in (ASC, DESC):
        for base in (LOCAL, GLOBAL):
            c.run_modes(order, base)


# ---------------------------------------------------------------------------------------------
# 2. tile edges: exactly G_k, G_k + 1 and 2 G_k - 1 segments of one class, lengths mixed within the class
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 12])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_tile_edges(dev, name, k):
    g = CAP >> k
    lo, hi = (1, 2) if k == 1 else (2 ** (k - 1) + 1, 2 ** k)
    for count in (g, g + 1, 2 * g - 1):
        rng = np.random.default_rng(100 * k + count)
        lens = rng.integers(lo, hi + 1, size=count)
        lens[0], lens[-1] = hi, lo
        c = make_case(dev, name, lens, seed=k + count)
        try:
            c.run_modes(ASC if count % 2 else DESC, GLOBAL if k == 5 else LOCAL)
        finally:
            c.release()


# ---------------------------------------------------------------------------------------------
# 3. few workgroups walk the tiles of all classes across class boundaries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 2])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_few_workgroups_walk_tiles_across_classes(dev, edge_cases, name, grid):
    dev.setParam("debug.sort_segments_grid", grid)
    try:
        assert dev.getParam("debug.sort_segments_grid") == grid
        edge_cases[name].run_modes(DESC if grid == 1 else ASC, GLOBAL)
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 4. ties and special values
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "u64"])
def test_all_equal_keys_give_the_identity_per_segment(dev, name):
    udt = BY_NAME[name][3]
    lens = [0, 7, 1, 300, 0, 0, 33, 4096, 2, 0]
    c = make_case(dev, name, lens, bits=lambda n: np.full(n, 0x3f800000, dtype=udt))
    try:
        ident = np.concatenate([np.arange(x) for x in lens])
        for order in (ASC, DESC):
            assert np.array_equal(c.expected(order)[0], ident)
            kernel = c.run_modes(order)
            dev.setParam("sort.segments_algo", FLAT)
            assert c.run_modes(order) == kernel
            dev.setParam("sort.segments_algo", AUTO)
    finally:
        reset(dev)
        c.release()


@pytest.mark.parametrize("case", ["nan30", "zeros_infs"])
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_float_cases_of_typed_shapes(dev, name, case):
    lens = [0, 5, 129, 0, 1000, 31, 32, 33, 2049, 1, 0]
    c = make_case(dev, name, lens, bits=lambda n: shape(name, case, n, seed=7))
    try:
        for order in (ASC, DESC):
            kernel = c.run_modes(order, GLOBAL)
            dev.setParam("sort.segments_algo", FLAT)
            assert c.run_modes(order, GLOBAL) == kernel
            dev.setParam("sort.segments_algo", AUTO)
    finally:
        reset(dev)
        c.release()


# ---------------------------------------------------------------------------------------------
# 5. degenerate shapes, on both paths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [[100], [0] * 20 + [77] + [0] * 29, [1] * 300, [1], [0, 1, 0]],
                         ids=["one_segment", "all_empty_but_one", "all_of_length_1", "n_1", "n_1_between_empties"])
def test_degenerate_shapes(dev, lens):
    try:
        for i, name in enumerate(("i32", "f64")):
            c = make_case(dev, name, lens, seed=len(lens) + i)
            try:
                for algo in (KERNEL, FLAT):
                    dev.setParam("sort.segments_algo", algo)
                    c.run_modes(DESC if i else ASC, GLOBAL if algo == KERNEL else LOCAL)
            finally:
                c.release()
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 6. the flat path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TYPE_IDS)
def test_flat_path_gives_the_kernel_path_bit_for_bit(dev, edge_cases, name):
    c = edge_cases[name]
    try:
        for order, base in ((ASC, GLOBAL), (DESC, LOCAL)):
            dev.setParam("sort.segments_algo", KERNEL)
            a = c.run_modes(order, base)
            dev.setParam("sort.segments_algo", FLAT)
            assert scratch_bytes(dev, c.kt, c.n, c.S, CAP) > 16 * c.n
            b = c.run_modes(order, base)
            assert a == b, "the two paths disagree"
    finally:
        reset(dev)


@pytest.mark.parametrize("name", ["f32", "i64"])
def test_flat_path_by_default_without_a_bound_or_above_4096(dev, name):
    assert dev.getParam("sort.segments_algo") == AUTO
    c = make_case(dev, name, [5000, 0, 7, 4097], seed=5000)
    try:
        for bound in (0, 5000):
            assert scratch_bytes(dev, c.kt, c.n, c.S, bound) > 16 * c.n   # (the flat path's four arrays)
            for order in (ASC, DESC):
                c.run_modes(order, GLOBAL if bound else LOCAL, bound=bound)
    finally:
        c.release()


@pytest.mark.parametrize("S", [1, 16, 17])
def test_flat_path_where_the_bits_of_the_segment_id_cross_a_multiple_of_4(dev, S):
    dev.setParam("sort.segments_algo", FLAT)
    try:
        for i, name in enumerate(("f32", "u64")):
            lens = np.random.default_rng(S).integers(0, 40, size=S)
            lens[-1] = 3
            ties = make_case(dev, name, lens, bits=lambda n: np.random.default_rng(S).integers(0, 3, size=n).astype(BY_NAME[name][3]))
            c = make_case(dev, name, lens, seed=S + i)
            try:
                for order in (ASC, DESC):
                    c.run_modes(order, LOCAL, bound=0)
                    ties.run_modes(order, GLOBAL)
            finally:
                c.release()
                ties.release()
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 7. a wrong bound is a defined result; offsets that break the contract stay inside the arrays
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_wrong_bound_passes_the_segment_through_and_counts_it(dev, name):
    dev.setParam("sort.segments_algo", KERNEL)
    wrong = make_case(dev, name, [3, 4097, 5], seed=4097)
    right = make_case(dev, name, [3, 4096, 5], seed=4096)
    try:
        for order in (ASC, DESC):
            for base in (LOCAL, GLOBAL):
                wrong.run_modes(order, base, bound=CAP, want_oversized=1, passthrough=(1,))
                right.run_modes(order, base, bound=CAP, want_oversized=0)
    finally:
        reset(dev)
        wrong.release()
        right.release()


@pytest.mark.parametrize("algo", [KERNEL, FLAT], ids=["kernel", "flat"])
@pytest.mark.parametrize("bad", [[0, 600, 200, 1000], [0, 300, 600, 1500], [5000, 4000, 0xffffffff, 0], [1000, 1000, 1000, 999]],
                         ids=["descending_pair", "last_above_n", "wild", "first_not_0"])
def test_bad_offsets_stay_inside_the_arrays(dev, algo, bad):
    dev.setParam("sort.segments_algo", algo)
    try:
        for name in ("f32", "u64"):
            bits = random_bits(BY_NAME[name][3], 1000, seed=3)
            c = Case(dev, name, bits, [400, 300, 300], device_offsets=bad)
            try:
                for order, base in ((ASC, LOCAL), (DESC, GLOBAL)):
                    c.run_modes(order, base, bound=1000 if algo == FLAT else 1000 // 2)
            finally:
                c.release()
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 8. the scratch query, the refusals, the knobs
# ---------------------------------------------------------------------------------------------
def test_scratch_query_matches_its_formula(dev):
    lib = _lib.load()

    def up(x):
        return (x + 255) // 256 * 256

    def w_argsort(m):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_sort_typed_scratch_bytes(dev._h, 2, 2, 0, m, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib_err()
        return c.value

    def w_soa32(m, bits):
        a, b, c = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.adlhip_radix_sort_soa_scratch_bytes(dev._h, 4, 4, m, bits, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0, lib_err()
        return c.value

    for n, S in ((1000, 1), (1000, 16), (1000, 17), (70001, 300), (5, 70001)):
        for kt in (2, 4):
            assert scratch_bytes(dev, kt, n, S, 100) == 4 * up(4 * S) + 256 + w_soa32(S, 4)
            bits = 4
            while (S - 1) >> bits:
                bits += 4
            flat = w_argsort(n) if S == 1 else 4 * up(4 * n) + max(w_argsort(n), w_soa32(n, bits))
            assert scratch_bytes(dev, kt, n, S, 0) == flat and scratch_bytes(dev, kt, n, S, CAP + 1) == flat
    assert scratch_bytes(dev, 2, 0, 5, 100) == 0 and scratch_bytes(dev, 2, 100, 0, 0) == 0


def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    F32 = 2
    call = lib.adlhip_sort_segments_typed
    sz = ctypes.c_size_t()
    lens = [40, 0, 100, 60]
    n, S = 200, 4
    for algo, bound in ((KERNEL, 100), (FLAT, 100), (AUTO, 0)):
        dev.setParam("sort.segments_algo", algo)
        wb = scratch_bytes(dev, F32, n, S, bound)
        inp = Framed(dev, payload=random_bits(np.uint32, n, seed=71), seed=1)
        off = Framed(dev, payload=np.concatenate([offsets_of(lens), np.zeros(3, np.uint32)]), seed=5)
        ko = Framed(dev, payload=np.arange(n, dtype=np.uint32) ^ np.uint32(0xa5a5a5a5), seed=2)
        io = Framed(dev, payload=np.arange(n, dtype=np.uint32) ^ np.uint32(0x5a5a5a5a), seed=3)
        cw = Framed(dev, nbytes=16, fill=0x5c, seed=6)
        w = Framed(dev, nbytes=wb, fill=0xa7, seed=4)
        h = dev._h

        def refused(rc, *words):
            assert rc == 1, words
            msg = lib_err()
            for word in words:
                assert word in msg, (words, msg)

        try:
            a = (inp.ptr(), n, off.ptr(), S, bound, LOCAL, ko.ptr(), io.ptr(), cw.ptr(), w.ptr(), wb)

            def but(**kw):
                names = ("keys", "n", "off", "S", "bound", "base", "ko", "io", "cw", "w", "wb")
                return tuple(kw.get(k, v) for k, v in zip(names, a))

            refused(call(h, F32, ASC, *but(keys=None)), "d_keys_in", "NULL")
            refused(call(h, F32, ASC, *but(off=None)), "d_offsets", "NULL")
            refused(call(h, F32, ASC, *but(w=None)), "d_work", "NULL")
            refused(call(h, F32, ASC, *but(ko=None, io=None)), "d_keys_out", "d_index_out")
            refused(call(h, F32, ASC, *but(keys=inp.ptr(4), n=n - 1)), "d_keys_in", "16-byte")
            refused(call(h, F32, ASC, *but(off=off.ptr(4))), "d_offsets", "16-byte")
            refused(call(h, F32, ASC, *but(ko=ko.ptr(4))), "d_keys_out", "16-byte")
            refused(call(h, F32, ASC, *but(io=io.ptr(8))), "d_index_out", "16-byte")
            refused(call(h, F32, ASC, *but(w=w.ptr(4))), "d_work", "16-byte")
            refused(call(h, F32, ASC, *but(cw=cw.ptr(2))), "d_num_oversized_out", "4-byte")
            refused(call(h, F32, ASC, *but(ko=inp.ptr(16))), "d_keys_out", "overlap", "d_keys_in")
            refused(call(h, F32, ASC, *but(io=inp.ptr(4 * (n - 4)))), "d_index_out", "overlap", "d_keys_in")
            refused(call(h, F32, ASC, *but(io=off.ptr(16))), "d_index_out", "overlap", "d_offsets")
            refused(call(h, F32, ASC, *but(ko=off.ptr(0))), "d_keys_out", "overlap", "d_offsets")
            refused(call(h, F32, ASC, *but(cw=inp.ptr(8))), "d_num_oversized_out", "overlap", "d_keys_in")
            refused(call(h, F32, ASC, *but(cw=off.ptr(4 * S))), "d_num_oversized_out", "overlap", "d_offsets")
            for bad in (-1, 6, 99):
                refused(call(h, bad, ASC, *a), "key_type")
                refused(lib.adlhip_sort_segments_scratch_bytes(h, bad, n, S, bound, ctypes.byref(sz)), "key_type")
            for bad in (-1, 2):
                refused(call(h, F32, bad, *a), "order")
                refused(call(h, F32, ASC, *but(base=bad)), "index_base")
            refused(call(h, F32, ASC, *but(n=1 << 32)), "n = ")
            refused(call(h, F32, ASC, *but(n=1 << 40)), "n = ")
            refused(call(h, F32, ASC, *but(S=1 << 32)), "num_segments")
            refused(lib.adlhip_sort_segments_scratch_bytes(h, F32, 1 << 32, S, bound, ctypes.byref(sz)), "n = ")
            refused(lib.adlhip_sort_segments_scratch_bytes(h, F32, n, 1 << 32, bound, ctypes.byref(sz)), "num_segments")
            refused(call(h, F32, ASC, *but(wb=wb - 1)), "work_bytes", str(wb))
            if algo == KERNEL:
                for bad in (0, CAP + 1):
                    refused(call(h, F32, ASC, *but(bound=bad)), "sort.segments_algo", "4096")
                    refused(lib.adlhip_sort_segments_scratch_bytes(h, F32, n, S, bad, ctypes.byref(sz)), "sort.segments_algo", "4096")
            assert ko.unchanged() and io.unchanged() and inp.unchanged() and w.unchanged() and cw.unchanged() and off.unchanged(), \
                "a refused call wrote something"
            # n == 0 and S == 0 succeed; they enqueue one 4-byte clear of the count word when it is given and nothing otherwise
            assert call(h, F32, DESC, *but(n=0, cw=None)) == 0, lib_err()
            assert call(h, F32, DESC, *but(S=0, cw=None)) == 0, lib_err()
            assert call(h, F32, DESC, None, 0, None, 0, bound, LOCAL, None, None, None, None, 0) == 0, lib_err()
            assert ko.unchanged() and io.unchanged() and inp.unchanged() and w.unchanged() and cw.unchanged() and off.unchanged()
            assert call(h, F32, DESC, *but(n=0, cw=cw.ptr(8))) == 0, lib_err()
            word = cw.read(np.uint32)
            assert word.tolist() == [0x5c5c5c5c, 0x5c5c5c5c, 0, 0x5c5c5c5c]
            assert call(h, F32, DESC, *but(S=0, cw=cw.ptr(4))) == 0, lib_err()
            assert cw.read(np.uint32).tolist() == [0x5c5c5c5c, 0, 0, 0x5c5c5c5c]
            assert ko.unchanged() and io.unchanged() and inp.unchanged() and w.unchanged() and off.unchanged()
            dev.checkFault()
            assert_idle(dev, "refusals")
        finally:
            reset(dev)
            for b in (inp, off, ko, io, cw, w):
                b.release()


def test_knobs_round_trip_and_leave_the_others_alone(dev):
    others = ["sort.rows_algo", "debug.sort_rows_grid", "topk.rows_algo", "debug.topk_rows_grid", "topk.algo", "sort.algo", "sort.mid",
              "unique.algo", "debug.unique_grid", "debug.search_grid", "sort.digit_bits"]
    before = [dev.getParam(k) for k in others]
    try:
        assert dev.getParam("sort.segments_algo") == -1 and dev.getParam("debug.sort_segments_grid") == 0
        for v in (0, 1, -1):
            dev.setParam("sort.segments_algo", v)
            assert dev.getParam("sort.segments_algo") == v
        for v in (1, 3, 100000, 0):
            dev.setParam("debug.sort_segments_grid", v)
            assert dev.getParam("debug.sort_segments_grid") == v
        for bad in (-2, 2, 17):
            with pytest.raises(Exception, match="sort.segments_algo"):
                dev.setParam("sort.segments_algo", bad)
        with pytest.raises(Exception, match="debug.sort_segments_grid"):
            dev.setParam("debug.sort_segments_grid", -1)
        assert dev.getParam("sort.segments_algo") == -1 and dev.getParam("debug.sort_segments_grid") == 0
        assert [dev.getParam(k) for k in others] == before
    finally:
        reset(dev)


# ---------------------------------------------------------------------------------------------
# 9. the Python mirror, torch, the facade
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    from oclradixsort_amd import Pprims
    p = Pprims()
    try:
        for lens, bound in (([6, 0, 607, 33, 0], 607), ([2, 6007, 0, 1], 0)):   # the segment kernel, the flat path
            offs = offsets_of(lens)
            n = int(offs[-1])
            bits = random_bits(np.uint64, n, seed=81 + n)
            keys, kout = Buffer(dev, n, np.float64), Buffer(dev, n, np.float64)
            ob, cnt = Buffer(dev, len(lens) + 1, np.uint32), Buffer(dev, 1, np.uint32)
            try:
                keys.write(bits.view(np.float64))
                ob.write(offs)
                cnt.write(np.array([77], np.uint32))
                out = p.sortSegments(dev, keys, ob, len(lens), maxSegment=bound, descending=True, keysOut=kout, globalIndex=True,
                                     oversizedOut=cnt)
                got = out.toHost().astype(np.int64)
                got_k = kout.toHost().view(np.uint64)
                out.release()
                want_i, want_k = expected_segments(bits, "f64", offs, DESC)
                want_i = want_i + np.repeat(offs[:-1].astype(np.int64), lens)
                assert np.array_equal(got, want_i) and np.array_equal(got_k, want_k) and cnt.toHost()[0] == 0
                dev.checkFault()
                assert_idle(dev, "Pprims.sortSegments")
            finally:
                for b in (keys, kout, ob, cnt):
                    b.release()
    finally:
        p.close()


@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


def _torch_input(dtype, n):
    g = torch.Generator(device="cuda").manual_seed(11)
    if dtype.is_floating_point:
        t = torch.randn(n, dtype=dtype, device="cuda", generator=g)
        return torch.where(t == 0, torch.ones_like(t), t)   # no -0 (and no +0 either), no NaN
    return torch.randint(-50, 50, (n,), dtype=dtype, device="cuda", generator=g)   # many ties


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_sort_segments_matches_torch(sorter, dtype_name, descending):
    dtype = getattr(torch, dtype_name)
    for lens, odt, on_device, bound in (([0, 5, 0, 0, 33, 1, 300, 0], torch.int64, True, None), ([7, 4097, 0, 2], torch.int32, False, None),
                                        ([100, 28, 0], torch.int32, True, 100), ([3, 4], torch.int64, True, 0), ([], torch.int64, False, None)):
        offs = offsets_of(lens).astype(np.int64)
        n = int(offs[-1])
        t = _torch_input(dtype, n + 1)[1:]   # contiguous, but it starts at an odd offset
        keep = t.clone()
        offsets = torch.tensor(offs, dtype=odt, device="cuda" if on_device else "cpu")
        cpu = t.cpu()
        want_v, want_i = torch.empty_like(cpu), torch.empty(n, dtype=torch.int64)
        for s in range(len(lens)):
            a, b = int(offs[s]), int(offs[s + 1])
            r = torch.sort(cpu[a:b], descending=descending, stable=True)
            want_v[a:b], want_i[a:b] = r.values, r.indices
        values, indices = sorter.sort_segments(t, offsets, descending=descending, max_segment=bound)
        only = sorter.argsort_segments(t, offsets, descending=descending, max_segment=bound, global_indices=True)
        torch.cuda.synchronize()
        assert values.dtype == dtype and indices.dtype == torch.int64 and only.dtype == torch.int64
        assert values.shape == t.shape and indices.shape == t.shape and only.shape == t.shape
        assert torch.equal(values.cpu(), want_v) and torch.equal(indices.cpu(), want_i)
        assert torch.equal(only.cpu(), want_i + torch.tensor(np.repeat(offs[:-1], np.asarray(lens, np.int64)), dtype=torch.int64))
        assert torch.equal(t, keep), "the input was changed"
    assert_idle(sorter.device, "TorchSorter.sort_segments")


def test_torch_sorter_sort_segments_refusals(sorter, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a native call was made")

    t = torch.arange(200, dtype=torch.int32, device="cuda")
    good = torch.tensor([0, 50, 200], device="cuda")
    monkeypatch.setattr(sorter.pprims, "sortSegments", boom)
    with torch.cuda.stream(torch.cuda.Stream()):
        with pytest.raises(RuntimeError):
            sorter.sort_segments(t, good)
    with pytest.raises(ValueError, match="1-D"):
        sorter.sort_segments(t.reshape(2, 100), good)
    with pytest.raises(TypeError):
        sorter.argsort_segments(t.to(torch.float16), good)
    with pytest.raises(ValueError):
        sorter.sort_segments(t.cpu(), good)
    with pytest.raises(ValueError, match="numel"):
        sorter.sort_segments(t, torch.tensor([0, 50, 199], device="cuda"))
    with pytest.raises(ValueError, match="numel"):
        sorter.sort_segments(t, torch.tensor([0, 50, 201]))
    with pytest.raises(ValueError, match="numel"):
        sorter.sort_segments(t, torch.tensor([1, 50, 200], device="cuda"))
    with pytest.raises(TypeError, match="int32 or int64"):
        sorter.sort_segments(t, torch.tensor([0.0, 200.0], device="cuda"))
    with pytest.raises(ValueError, match="num_segments"):
        sorter.sort_segments(t, good.reshape(1, 3))
    with pytest.raises(TypeError):
        sorter.sort_segments(t, [0, 200])
    monkeypatch.undo()
    values, indices = sorter.sort_segments(t, good, descending=True, global_indices=True)
    assert values[:3].tolist() == [49, 48, 47] and indices[50:53].tolist() == [199, 198, 197]


def test_sort_segments_demo_on_the_device_prints_what_the_host_path_prints():
    def lines(args):
        r = subprocess.run([DEMO, "--dump"] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.startswith("[") or ln.startswith("DUMP ")]

    device, host = lines([]), lines(["--host"])
    assert len(device) == 12 * 6 + 12 * 4 and all(ln.startswith("[ OK ] SortSegments.") for ln in device if ln.startswith("["))
    assert device == host
