"""Join of sorted sequences and expansion of runs on the GPU (include/adlhip.h "expansion of runs and join of sorted sequences";
oclradixsort_amd/csrc/join_kernels.hpp; Pprims.joinSorted / expandRuns; TorchSorter.join / repeat_interleave).

The oracle is tests/join_oracle.py (numpy: a searchsorted on the codes, then np.repeat; tests/test_join_api.py checks it against a
double loop over all pairs).  Every case is compared bit for bit: the 64-bit count word, and the first min(T, cap) rows of every output.

Every output is sized exactly cap elements, prefilled with sentinels and read back whole: elements [min(T, cap), cap) and the guard bytes
behind cap must be untouched.  Every input and the work buffer (sized exactly the reported bytes and prefilled with junk) carry guard
bytes too, and the inputs are compared with their originals afterwards.  The handle's device state is idle after each case.

T is the tile of the join and the expansion: 2048 items -- elements of A, or elements plus rows.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

import large_n as L
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from join_oracle import (ANTI, ASC, BY_NAME, DESC, INNER, KINDS, LEFT, NONE, SEMI, SPECIALS, TYPE_IDS, codes, expand_oracle, is_sorted,
                         join_oracle, join_total, sort_bits)
from test_gpu_merge import Padded
from test_gpu_reduce import Guarded, lib_err, random_bits, sentinels

pytestmark = pytest.mark.gpu

T = 2048
ALL_KINDS = (INNER, LEFT, SEMI, ANTI)
GRIDS = [0, 1, 3]
ORDERS = [ASC, DESC]
SENTINELS = 64
UDT = {0: None, 4: np.uint32, 8: np.uint64}
COUNT_SENTINEL = np.array([0xdeadbeefcafef00d], np.uint64)
LIMIT = 0xFFF00000


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.join_grid", 0)
    DeviceUtils.deallocate(d)


def join_bytes(dev, key_type, na, nb, cap):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_join_scratch_bytes(dev._h, key_type, na, nb, cap, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def expand_bytes(dev, n, cap):
    wb = ctypes.c_size_t()
    rc = _lib.load().adlhip_expand_scratch_bytes(dev._h, n, cap, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def caps_of(total):
    """the five capacities of the issue: counting only, 1, T - 1, T, T + 100 (T here: the oracle's row count)"""
    return sorted({0, 1, max(total - 1, 0), total, total + 100})


class Outs:
    """the outputs of one call: sentinel-filled arrays of exactly cap elements, a guarded 8-byte count word, a work buffer of exactly
    the reported bytes prefilled with junk.  outs: {name: dtype}"""

    def __init__(self, dev, outs, cap, work_bytes, fill=0xff):
        self.dev, self.cap = dev, cap
        self.sent = {k: sentinels(dt, cap, 0xa5a5a5a5a5a5a5a5 + 77 * i) for i, (k, dt) in enumerate(outs.items())} if cap else {}
        self.g = {k: Guarded(dev, s, guard_bytes=SENTINELS * s.dtype.itemsize, seed=20 + i) for i, (k, s) in enumerate(self.sent.items())}
        self.count = Guarded(dev, COUNT_SENTINEL, guard_bytes=64, seed=3)
        self.work = Guarded(dev, nbytes=work_bytes, seed=9, fill=fill)

    def ptr(self, name):
        return self.g[name].ptr() if name in self.g else None

    def check(self, exp, total, what):
        """exp: {name: at least the first min(total, cap) expected elements}"""
        got = int(self.count.read(np.uint64)[0])
        assert got == total, "%s: the count word says %d, expected %d" % (what, got, total)
        r = min(total, self.cap)
        for k, g in self.g.items():
            x = g.read(self.sent[k].dtype)
            e = exp[k][:r]
            if not np.array_equal(x[:r], e):
                bad = np.flatnonzero(x[:r] != e)
                raise AssertionError("%s: %s differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                    what, k, bad.size, r, bad[0], int(x[bad[0]]), int(e[bad[0]])))
            assert np.array_equal(x[r:], self.sent[k][r:]), "%s: %s was written at row %d or beyond" % (what, k, r)
        self.work.check_guard()
        assert self.dev.getParam("debug.idle_dirty") == 0

    def untouched(self):
        assert int(self.count.read(np.uint64)[0]) == COUNT_SENTINEL[0], "the count word was written"
        for k, g in self.g.items():
            assert np.array_equal(g.read(self.sent[k].dtype), self.sent[k]), "%s was written" % k

    def release(self):
        for b in list(self.g.values()) + [self.count, self.work]:
            b.release()


def call_join(dev, kname, order, kind, pa, na, pb, nb, cap, o, **over):
    arg = dict(key_type=BY_NAME[kname][1], order=order, kind=kind, a=pa, na=na, b=pb, nb=nb, cap=cap, ia=o.ptr("a"), ib=o.ptr("b"),
               num=o.count.ptr(), work=o.work.ptr(), work_bytes=o.work.nbytes)
    arg.update(over)
    return _lib.load().adlhip_join_sorted_typed(dev._h, arg["key_type"], arg["order"], arg["kind"], arg["a"], arg["na"], arg["b"], arg["nb"],
                                                arg["cap"], arg["ia"], arg["ib"], arg["num"], arg["work"], arg["work_bytes"])


def run_join(dev, kname, a, b, kinds=ALL_KINDS, orders=(ASC,), grids=(0,), caps=None, off=(0, 0), fill=0xff, form=("a", "b"), presorted=False):
    """adlhip_join_sorted_typed on a and b, each sorted here in every order asked, for every kind, capacity (caps: a function of the
    oracle's row count; default: exactly that count) and grid, with every check of the memory contract.  Returns {(order, kind): T}"""
    res = {}
    for order in orders:
        sa, sb = (a, b) if presorted else (sort_bits(a, kname, order), sort_bits(b, kname, order))
        assert is_sorted(sa, kname, order) and is_sorted(sb, kname, order)
        ins = {"a": Padded(dev, sa, off[0], 5), "b": Padded(dev, sb, off[1], 6)}
        try:
            for kind in kinds:
                ia, ib, total = join_oracle(sa, sb, kname, kind, order)
                res[(order, kind)] = total
                for cap in (caps(total) if caps else (total,)):
                    odt = {k: np.uint32 for k in form} if cap else {}
                    o = Outs(dev, odt, cap, join_bytes(dev, BY_NAME[kname][1], sa.size, sb.size, cap), fill=fill)
                    try:
                        for grid in grids:
                            dev.setParam("debug.join_grid", grid)
                            what = "%s %s order %d na %d nb %d cap %d of %d grid %d off %s" % (KINDS[kind], kname, order, sa.size, sb.size,
                                                                                               cap, total, grid, off)
                            rc = call_join(dev, kname, order, kind, ins["a"].ptr(), sa.size, ins["b"].ptr(), sb.size, cap, o)
                            assert rc == 0, what + ": " + lib_err()
                            o.check({"a": ia, "b": ib}, total, what)
                    finally:
                        o.release()
            for k, p in ins.items():
                assert p.unchanged(), "input %s was changed" % k
        finally:
            dev.setParam("debug.join_grid", 0)
            for p in ins.values():
                p.release()
    return res


# ---------------------------------------------------------------------------------------------
# sizes x kinds x grids
# ---------------------------------------------------------------------------------------------
NAS = [0, 1, T - 1, T, T + 1, 3 * T + 5]
NBS = NAS + [4097, 10000]          # the last two: the table of B is every second and every third element, the search has two levels


@pytest.mark.parametrize("na", NAS)
def test_sizes_kinds_and_grids(dev, na):
    rng = np.random.default_rng(1000 + na)
    for j, nb in enumerate(NBS):
        # a third as many distinct keys as elements: runs inside an input, across the inputs and across tile boundaries
        a, b = (rng.integers(0, max(na, nb) // 3 + 2, size=m).astype(np.uint32) for m in (na, nb))
        for kind in ALL_KINDS:
            run_join(dev, "i32", a, b, kinds=(kind,), grids=(GRIDS[(j + kind) % 3],))
    a, b = (rng.integers(0, na // 3 + 2, size=m).astype(np.uint64) for m in (na, 10000))
    run_join(dev, "f64", a, b, orders=(DESC,), grids=GRIDS)


def test_more_tiles_than_one_chunk_on_the_default_grid(dev):
    """8 workgroups per CU take one tile each up to 8 x CUs tiles; beyond that a chunk is several tiles"""
    tiles = 8 * int(dev.info.compute_units) + 5
    na = tiles * T + 3
    rng = np.random.default_rng(23)
    a, b = (rng.integers(0, na // 2, size=m).astype(np.uint32) for m in (na, na // 4))
    run_join(dev, "u32", a, b, kinds=(INNER, LEFT))


# ---------------------------------------------------------------------------------------------
# types, orders, kinds, offsets
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS, ids=["asc", "desc"])
@pytest.mark.parametrize("kname", TYPE_IDS)
def test_every_key_type_order_and_kind_with_special_patterns(dev, kname, order):
    udt = BY_NAME[kname][3]
    w = np.dtype(udt).itemsize
    na, nb = T + 300, T + 500
    rng = np.random.default_rng(400 + BY_NAME[kname][1])
    pool = np.concatenate([random_bits(udt, 300, rng), SPECIALS[w]])          # both inputs draw from one pool: shared keys, duplicates
    a, b = pool[rng.integers(0, pool.size, size=na)], pool[rng.integers(0, pool.size, size=nb)]
    for x in (a, b):                                      # specials that repeat, in both inputs (+-0, +-inf, NaN payloads)
        x[rng.integers(0, x.size, size=x.size // 3)] = SPECIALS[w][rng.integers(0, SPECIALS[w].size, size=x.size // 3)]
    run_join(dev, kname, a, b, orders=(order,), grids=(0, 1))
    for off in ((1, 3), (3, 1)):
        run_join(dev, kname, a, b, kinds=(INNER, LEFT), orders=(order,), grids=(0, 3), off=off)
    run_join(dev, kname, a, b, kinds=(INNER, ANTI), orders=(order,), form=("a",))      # one output alone
    run_join(dev, kname, a, b, kinds=(LEFT,), orders=(order,), form=("b",))


def test_a_and_b_the_same_array(dev):
    """A == B, the same pointer: every run of m elements gives m x m rows"""
    rng = np.random.default_rng(72)
    a = sort_bits(rng.integers(0, 500, size=2 * T + 5).astype(np.uint64), "i64", DESC)
    p = Padded(dev, a, 1, 5)
    try:
        for kind in ALL_KINDS:
            ia, ib, total = join_oracle(a, a, "i64", kind, DESC)
            assert total == (0 if kind == ANTI else a.size if kind == SEMI else int((np.unique(a, return_counts=True)[1].astype(np.int64) ** 2).sum()))
            o = Outs(dev, {"a": np.uint32, "b": np.uint32}, total, join_bytes(dev, 4, a.size, a.size, total))
            try:
                assert call_join(dev, "i64", DESC, kind, p.ptr(), a.size, p.ptr(), a.size, total, o) == 0, lib_err()
                o.check({"a": ia, "b": ib}, total, "B is A, %s" % KINDS[kind])
            finally:
                o.release()
        assert p.unchanged()
    finally:
        p.release()


# ---------------------------------------------------------------------------------------------
# skew
# ---------------------------------------------------------------------------------------------
X = 0x40000000


def _skew_cases():
    u = np.uint32
    lows = lambda k: np.arange(k, dtype=u) * u(2)                  # noqa: E731  (distinct even keys below X)
    odds = lambda k: np.arange(k, dtype=u) * u(2) + u(1)           # noqa: E731  (distinct odd keys below X: none of them in lows)
    run = lambda k: np.full(k, X, u)                               # noqa: E731
    return {
        "one_key_3_x_5000": (run(3), run(5000)),
        "one_key_5000_x_3": (run(5000), run(3)),
        "one_key_300_x_300": (run(300), run(300)),
        # 5000 elements of A without a match, then one with 5000 matches; and the mirror image
        "5000_unmatched_then_5000_matches": (np.concatenate([odds(5000), run(1)]), np.concatenate([lows(700), run(5000)])),
        "5000_matches_then_5000_unmatched": (np.concatenate([run(1), odds(5000) + u(X)]), np.concatenate([run(5000), lows(700) + u(X + 2)])),
        "all_of_a_unmatched": (odds(3 * T + 5), lows(T + 9)),
        "all_of_a_equal_b_empty": (run(T + 7), run(0)),
    }


SKEW_CASES = _skew_cases()


@pytest.mark.parametrize("name", sorted(SKEW_CASES))
def test_skew(dev, name):
    a, b = SKEW_CASES[name]
    res = run_join(dev, "u32", a, b, orders=ORDERS, grids=GRIDS, presorted=False)
    run_join(dev, "u64", a.astype(np.uint64) << np.uint64(20), b.astype(np.uint64) << np.uint64(20), kinds=(INNER, LEFT), grids=(0, 3))
    want = {"one_key_3_x_5000": (15000, 15000, 3, 0), "one_key_5000_x_3": (15000, 15000, 5000, 0), "one_key_300_x_300": (90000, 90000, 300, 0),
            "5000_unmatched_then_5000_matches": (5000, 10000, 1, 5000), "5000_matches_then_5000_unmatched": (5000, 10000, 1, 5000),
            "all_of_a_unmatched": (0, 3 * T + 5, 0, 3 * T + 5), "all_of_a_equal_b_empty": (0, T + 7, 0, T + 7)}[name]
    for order in ORDERS:
        assert tuple(res[(order, k)] for k in ALL_KINDS) == want


# ---------------------------------------------------------------------------------------------
# capacity; the 64-bit count
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS, ids=KINDS)
def test_every_capacity_against_the_row_count(dev, kind):
    rng = np.random.default_rng(300 + kind)
    a, b = (rng.integers(0, 900, size=m).astype(np.uint32) for m in (2 * T + 9, T + 77))
    res = run_join(dev, "f32", a, b, kinds=(kind,), orders=ORDERS, grids=GRIDS, caps=caps_of)
    assert all(t > 100 for t in res.values())
    # a row count that is a whole number of tiles of elements plus rows, and one more and one less: 3 * T elements, m rows each
    for extra in (-1, 0, 1):
        a = np.arange(3 * T, dtype=np.uint32)
        b = np.sort(np.concatenate([a, a[:T + extra]]))
        run_join(dev, "u32", a, b, kinds=(kind,), grids=(0, 3), caps=caps_of)


def test_a_count_beyond_2p32(dev):
    """na = nb = 65537 copies of one key: T = 65537^2 = 4 295 098 369 > 2^32; counting only, and with cap = 4096: rows (0, 0 .. 4095)"""
    n = 65537
    a = np.full(n, 7, np.uint32)
    p = Padded(dev, a, 0, 5)
    try:
        for kind, total in ((INNER, n * n), (LEFT, n * n), (SEMI, n), (ANTI, 0)):
            assert join_total(a, a, "u32", kind) == total
            for cap in (0, 4096):
                ia, ib, _ = join_oracle(a, a, "u32", kind, limit=cap)
                o = Outs(dev, {"a": np.uint32, "b": np.uint32} if cap else {}, cap, join_bytes(dev, 0, n, n, cap))
                try:
                    for grid in (0, 3):
                        dev.setParam("debug.join_grid", grid)
                        assert call_join(dev, "u32", ASC, kind, p.ptr(), n, p.ptr(), n, cap, o) == 0, lib_err()
                        o.check({"a": ia, "b": ib}, total, "65537 x 65537 %s cap %d" % (KINDS[kind], cap))
                    if cap and kind == INNER:
                        assert not ia.any() and np.array_equal(ib, np.arange(4096, dtype=np.uint32))
                finally:
                    dev.setParam("debug.join_grid", 0)
                    o.release()
        assert p.unchanged()
    finally:
        p.release()


# ---------------------------------------------------------------------------------------------
# the work buffer, refusals, empty input
# ---------------------------------------------------------------------------------------------
def test_work_buffer_contents_do_not_matter(dev):
    rng = np.random.default_rng(81)
    a, b = (rng.integers(0, 1500, size=m).astype(np.uint64) for m in (2 * T + 9, T + 1))
    for fill in (0x00, 0xff, 0x5a):
        run_join(dev, "f64", a, b, kinds=(INNER, LEFT), grids=(0, 3), fill=fill)


def test_scratch_bytes_follow_the_formulas(dev):
    up = lambda x: (x + 255) // 256 * 256     # noqa: E731
    chunks = up(8 * 8 * int(dev.info.compute_units))
    for na, nb, cap in ((0, 0, 0), (1, 0, 0), (T, 1, 0), (T, 1, 1), (1000, 5 * T, 63 * T), (63 * T, 1, T + 1), (1 << 31, 5, LIMIT - (1 << 31)),
                        (5, LIMIT - 5, 0)):
        tiles = (na + cap + T - 1) // T
        for kt in (0, 5, 2):
            assert join_bytes(dev, kt, na, nb, cap) == chunks + 2 * up(4 * na) + up(4 * (tiles + 1)), (na, nb, cap)
        assert expand_bytes(dev, na, cap) == chunks + up(4 * na) + up(4 * (tiles + 1)), (na, cap)
    sz = ctypes.c_size_t()
    lib = _lib.load()
    for args in ((0, 1 << 31, LIMIT + 1 - (1 << 31), 0), (0, LIMIT + 1, 0, 0), (0, 5, 5, LIMIT - 4), (0, 1 << 40, 0, 0), (0, 0, 0, 1 << 40),
                 (0, (1 << 64) - 1, 2, 0), (0, 2, 0, (1 << 64) - 1), (6, 5, 5, 0), (-1, 5, 5, 0)):
        assert lib.adlhip_join_scratch_bytes(dev._h, *args, ctypes.byref(sz)) == 1, args
        assert lib_err()
    for args in ((LIMIT + 1, 0), (5, LIMIT - 4), ((1 << 64) - 1, 2), (0, 1 << 40)):
        assert lib.adlhip_expand_scratch_bytes(dev._h, *args, ctypes.byref(sz)) == 1, args
        assert lib_err()


def test_join_refusals_enqueue_nothing(dev):
    rng = np.random.default_rng(91)
    na, nb, cap = 3000, 2000, 5000
    a, b = sort_bits(rng.integers(0, 2500, size=na).astype(np.uint32), "u32", ASC), sort_bits(rng.integers(0, 2500, size=nb).astype(np.uint32), "u32", ASC)
    pa, pb = Padded(dev, a, 0, 5), Padded(dev, b, 0, 6)
    o = Outs(dev, {"a": np.uint32, "b": np.uint32}, cap, join_bytes(dev, 0, na, nb, cap))
    wb = o.work.nbytes
    null = ctypes.c_void_p(0)

    def refused(what, *names, **over):
        rc = call_join(dev, "u32", over.pop("order", ASC), over.pop("kind", INNER), over.pop("a", pa.ptr()), over.pop("na", na),
                       over.pop("b", pb.ptr()), over.pop("nb", nb), over.pop("cap", cap), o, **over)
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        for name in names:
            assert name in msg, (what, msg)
        return msg

    try:
        for bad in (-1, 4, 99):
            refused("kind %d" % bad, "kind", kind=bad)
        for bad in (-1, 6, 99):
            refused("key_type %d" % bad, "key_type", key_type=bad)
        for bad in (-1, 2):
            refused("order %d" % bad, "order", order=bad)
        refused("NULL keys of A", "d_keys_a", a=null)
        refused("NULL keys of B", "d_keys_b", b=null)
        refused("NULL count word", "d_num_out", num=null)
        refused("NULL work", "d_work", work=null)
        refused("cap > 0 with no output", "d_index_a_out", "d_index_b_out", ia=null, ib=null)
        refused("outputs with cap 0", "cap", cap=0)
        refused("one output with cap 0", "cap", cap=0, ia=null)
        refused("misaligned keys of A", "d_keys_a", a=ctypes.c_void_p(pa.ptr().value + 2))
        refused("misaligned keys of B", "d_keys_b", b=ctypes.c_void_p(pb.ptr().value + 1))
        refused("misaligned index a", "d_index_a_out", ia=o.g["a"].ptr(4), cap=cap - 1)
        refused("misaligned index b", "d_index_b_out", ib=o.g["b"].ptr(8), cap=cap - 2)
        refused("misaligned count word", "d_num_out", num=o.count.ptr(4))
        refused("misaligned work", "d_work", work=o.work.ptr(4), work_bytes=wb - 4)
        refused("index a is keys of A", "d_index_a_out", "d_keys_a", ia=pa.ptr(), cap=na)
        refused("index b overlaps the end of B", "d_index_b_out", "d_keys_b", ib=pb.ptr(nb - 4), cap=4)
        refused("index b overlaps index a", "d_index_a_out", "d_index_b_out", ib=o.g["a"].ptr(16), cap=cap - 4)
        refused("the count word lies in the keys of B", "d_num_out", "d_keys_b", num=pb.ptr(8))
        refused("the count word lies in index a", "d_index_a_out", "d_num_out", num=o.g["a"].ptr(64))
        refused("the work buffer is the keys of A", "d_work", "d_keys_a", work=pa.ptr(), work_bytes=4 * na)
        refused("na + nb beyond the limit", "na + nb", na=LIMIT + 1 - nb)
        refused("na + nb = 2^32", "na + nb", na=1 << 31, nb=1 << 31)
        refused("na beyond size_t's half", "na + nb", na=(1 << 64) - 1, nb=2)
        refused("na + cap beyond the limit", "na + cap", cap=LIMIT + 1 - na)
        refused("cap beyond size_t's half", "na + cap", cap=(1 << 64) - 1)
        msg = refused("work one byte short", "adlhip_join_scratch_bytes", work_bytes=wb - 1)
        assert str(wb) in msg
        o.untouched()
        assert pa.unchanged() and pb.unchanged()
        assert dev.getParam("debug.idle_dirty") == 0
        # the proper calls go through
        for kind in ALL_KINDS:
            ia, ib, total = join_oracle(a, b, "u32", kind, limit=cap)
            assert call_join(dev, "u32", ASC, kind, pa.ptr(), na, pb.ptr(), nb, cap, o) == 0, lib_err()
            got = int(o.count.read(np.uint64)[0])
            assert got == total
            r = min(total, cap)
            assert np.array_equal(o.g["a"].read(np.uint32)[:r], ia) and np.array_equal(o.g["b"].read(np.uint32)[:r], ib)
    finally:
        for x in (pa, pb, o):
            x.release()


def test_empty_inputs(dev):
    a = np.arange(10, dtype=np.uint32)
    p = Padded(dev, a, 0, 5)
    o = Outs(dev, {"a": np.uint32, "b": np.uint32}, 16, join_bytes(dev, 0, 10, 10, 16))
    try:
        for kind in ALL_KINDS:
            # na == 0: only the clear of the count; no arrays and no work buffer needed
            for over in (dict(nb=10), dict(a=None, b=None, nb=0, work=None, work_bytes=0)):
                o.count.buf.write(COUNT_SENTINEL.view(np.uint8))
                assert call_join(dev, "u32", ASC, kind, over.pop("a", p.ptr()), 0, over.pop("b", p.ptr()), over.pop("nb"), 16, o, **over) == 0, lib_err()
                o.check({"a": a[:0], "b": a[:0]}, 0, "empty A")
            # nb == 0 (B not looked at): nothing for inner and semi, every element of A for left and anti
            ia, ib, total = join_oracle(a, a[:0], "u32", kind)
            assert total == (10 if kind in (LEFT, ANTI) else 0)
            assert call_join(dev, "u32", DESC, kind, p.ptr(), 10, None, 0, 16, o) == 0, lib_err()
            o.check({"a": ia, "b": ib}, total, "empty B")
            for k, s in o.sent.items():
                o.g[k].buf.write(s.view(np.uint8))
        # refusals come first even then
        o.count.buf.write(COUNT_SENTINEL.view(np.uint8))
        assert call_join(dev, "u32", ASC, INNER, p.ptr(), 0, p.ptr(), 0, 16, o, ia=None, ib=None) == 1
        assert call_join(dev, "u32", ASC, INNER, p.ptr(), 0, p.ptr(), 0, 16, o, key_type=7) == 1
        assert call_join(dev, "u32", ASC, 4, p.ptr(), 0, p.ptr(), 0, 16, o) == 1
        assert call_join(dev, "u32", ASC, INNER, p.ptr(), 0, p.ptr(), 0, 16, o, num=None) == 1
        o.untouched()
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        p.release()
        o.release()


# ---------------------------------------------------------------------------------------------
# inputs that are not sorted
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("na,nb", [(T + 1, 3 * T + 5), (3 * T + 7, 3), (2 * T, 10000)], ids=lambda v: str(v))
def test_unsorted_inputs_stay_inside_every_buffer(dev, na, nb, grid):
    """The rows and the count are unspecified; the call succeeds, the stream reports no fault, every written index_a is below na, every
    written index_b is below nb or is NONE, nothing is written at cap or beyond, every guard is intact and the inputs are unchanged
    (join_kernels.hpp, BOUNDS).  A valid call on valid buffers: this asserts memory safety."""
    rng = np.random.default_rng(900 + na + grid)
    dev.setParam("debug.join_grid", grid)
    try:
        for kname, span in (("f32", 1 << 32), ("i64", 50)):
            udt = BY_NAME[kname][3]
            a, b = (rng.integers(0, span, size=m).astype(udt) for m in (na, nb))
            pa, pb = Padded(dev, a, 1, 5), Padded(dev, b, 3, 6)
            try:
                for order in ORDERS:
                    for kind in ALL_KINDS:
                        for cap in (0, 700, 4 * na):
                            o = Outs(dev, {"a": np.uint32, "b": np.uint32} if cap else {}, cap, join_bytes(dev, BY_NAME[kname][1], na, nb, cap))
                            try:
                                assert call_join(dev, kname, order, kind, pa.ptr(), na, pb.ptr(), nb, cap, o) == 0, lib_err()
                                DeviceUtils.waitForCompletion(dev)        # adlhip_sync: raises on a device fault
                                total = int(o.count.read(np.uint64)[0])
                                o.count.check_guard()
                                o.work.check_guard()
                                if cap:
                                    r = min(total, cap)
                                    xa, xb = o.g["a"].read(np.uint32), o.g["b"].read(np.uint32)      # (checks the guards behind them)
                                    assert bool((xa[:r] < na).all()), "an index_a outside A"
                                    assert bool(((xb[:r] < nb) | (xb[:r] == NONE)).all()), "an index_b outside B"
                                    assert np.array_equal(xa[r:], o.sent["a"][r:]) and np.array_equal(xb[r:], o.sent["b"][r:])
                                assert dev.getParam("debug.idle_dirty") == 0
                            finally:
                                o.release()
                assert pa.unchanged() and pb.unchanged()
            finally:
                pa.release()
                pb.release()
    finally:
        dev.setParam("debug.join_grid", 0)


# ---------------------------------------------------------------------------------------------
# expand_runs
# ---------------------------------------------------------------------------------------------
def call_expand(dev, pc, n, vbytes, pv, cap, o, **over):
    arg = dict(counts=pc, n=n, value_bytes=vbytes, vals=pv, cap=cap, run=o.ptr("run"), rank=o.ptr("rank"), vout=o.ptr("vals"), num=o.count.ptr(),
               work=o.work.ptr(), work_bytes=o.work.nbytes)
    arg.update(over)
    return _lib.load().adlhip_expand_runs(dev._h, arg["counts"], arg["n"], arg["value_bytes"], arg["vals"], arg["cap"], arg["run"], arg["rank"],
                                          arg["vout"], arg["num"], arg["work"], arg["work_bytes"])


def run_expand(dev, counts, vbytes=0, grids=(0,), caps=None, off=0, form=("run", "rank", "vals"), limit=None):
    """adlhip_expand_runs on counts for every capacity and grid, with every check of the memory contract; limit: the oracle computes the
    rows of the counts capped so that their sum stays small (for sums beyond 2^32), the count is checked against the full sum"""
    rng = np.random.default_rng(counts.size + vbytes)
    vals = random_bits(UDT[vbytes], counts.size, rng) if vbytes else None
    form = tuple(k for k in form if k != "vals" or vbytes)
    full = int(counts.astype(np.int64).sum())
    if limit is None:
        run, rank, vout, total = expand_oracle(counts, vals)
    else:
        run, rank, vout, _ = expand_oracle(np.minimum(counts, limit), vals)      # the first `limit` rows are those of the full counts
        run, rank, vout, total = run[:limit], rank[:limit], vout[:limit] if vout is not None else None, full
    assert total == full
    pc = Padded(dev, counts, off, 5)
    pv = Padded(dev, vals, off, 6) if vbytes else None
    try:
        for cap in (caps(total) if caps else (total,)):
            assert limit is None or cap <= limit
            odt = {k: {"run": np.uint32, "rank": np.uint32, "vals": UDT[vbytes]}[k] for k in form} if cap else {}
            o = Outs(dev, odt, cap, expand_bytes(dev, counts.size, cap))
            try:
                for grid in grids:
                    dev.setParam("debug.join_grid", grid)
                    what = "expand runs %d value_bytes %d cap %d of %d grid %d off %d" % (counts.size, vbytes, cap, total, grid, off)
                    rc = call_expand(dev, pc.ptr(), counts.size, vbytes if "vals" in odt else 0, pv.ptr() if "vals" in odt else None, cap, o)
                    assert rc == 0, what + ": " + lib_err()
                    o.check({"run": run, "rank": rank, "vals": vout}, total, what)
            finally:
                o.release()
        assert pc.unchanged() and (pv is None or pv.unchanged())
    finally:
        dev.setParam("debug.join_grid", 0)
        pc.release()
        if pv is not None:
            pv.release()
    return total


@pytest.mark.parametrize("n", [0, 1, T - 1, T, T + 1])
def test_expand_sizes_values_and_capacities(dev, n):
    rng = np.random.default_rng(50 + n)
    counts = rng.integers(0, 4, size=n).astype(np.uint32)
    for vbytes, off in ((0, 0), (4, 1), (8, 3)):
        run_expand(dev, counts, vbytes, grids=GRIDS, caps=caps_of, off=off)
    if n:
        run_expand(dev, counts, 8, form=("vals",))
        run_expand(dev, counts, 0, form=("rank",))


def test_expand_zero_stretches_one_long_run_and_tile_multiples(dev):
    rng = np.random.default_rng(7)
    few = lambda k: rng.integers(0, 3, size=k).astype(np.uint32)       # noqa: E731
    # 5000 consecutive zero counts between runs that have rows
    run_expand(dev, np.concatenate([few(300), np.zeros(5000, np.uint32), few(300)]), 4, grids=GRIDS, caps=caps_of)
    # one count of 10000 among short runs, and alone
    run_expand(dev, np.concatenate([few(100), np.array([10000], np.uint32), few(100)]), 8, grids=GRIDS, caps=caps_of)
    run_expand(dev, np.array([10000], np.uint32), 4, grids=(0, 3))
    # runs + rows = exactly two tiles, and one more and one less: 1000 runs and 2 T - 1000 + extra rows
    for extra in (-1, 0, 1):
        counts = np.ones(1000, np.uint32)
        counts[-1] += 2 * T - 2000 + extra
        assert counts.size + int(counts.sum()) == 2 * T + extra
        run_expand(dev, counts, 4, grids=GRIDS, caps=caps_of)
        counts = np.full(T + extra, 1, np.uint32)                     # rows == runs: a tile holds as many of the one as of the other
        run_expand(dev, counts, 0, grids=(0, 3))


def test_expand_a_sum_beyond_2p32(dev):
    """three counts of 0x7FFFFFFF: T = 6 442 450 941 > 2^32; counting only, and cap = 4096: all of them rows of run 0"""
    counts = np.full(3, 0x7FFFFFFF, np.uint32)
    total = run_expand(dev, counts, 8, grids=(0, 3), caps=lambda t: (0, 4096), limit=4096)
    assert total == 3 * 0x7FFFFFFF > 1 << 32
    run_expand(dev, np.array([5, 0xFFFFFFFF, 0xFFFFFFFF, 9], np.uint32), 4, caps=lambda t: (0, 4096), limit=4096)


def test_expand_refusals_enqueue_nothing(dev):
    n, cap = 3000, 5000
    counts = np.random.default_rng(3).integers(0, 3, size=n).astype(np.uint32)
    vals = random_bits(np.uint64, n, np.random.default_rng(4))
    pc, pv = Padded(dev, counts, 0, 5), Padded(dev, vals, 0, 6)
    o = Outs(dev, {"run": np.uint32, "rank": np.uint32, "vals": np.uint64}, cap, expand_bytes(dev, n, cap))
    wb = o.work.nbytes
    null = ctypes.c_void_p(0)

    def refused(what, *names, **over):
        rc = call_expand(dev, over.pop("counts", pc.ptr()), over.pop("n", n), over.pop("value_bytes", 8), over.pop("vals", pv.ptr()),
                         over.pop("cap", cap), o, **over)
        assert rc == 1, what
        msg = lib_err()
        for name in names:
            assert name in msg, (what, msg)
        return msg

    try:
        refused("NULL counts", "d_counts_in", counts=null)
        refused("NULL values in with values out", "d_vals_in", vals=null)
        refused("NULL count word", "d_num_out", num=null)
        refused("NULL work", "d_work", work=null)
        for bad in (-1, 2, 16):
            refused("value_bytes %d" % bad, "value_bytes", value_bytes=bad)
        refused("value_bytes 0 with value arrays", "value_bytes", value_bytes=0)
        refused("cap > 0 with no output", "d_run_out", run=null, rank=null, vout=null)
        refused("outputs with cap 0", "cap", cap=0)
        refused("misaligned counts", "d_counts_in", counts=ctypes.c_void_p(pc.ptr().value + 2))
        refused("misaligned values", "d_vals_in", vals=ctypes.c_void_p(pv.ptr().value + 4))
        refused("misaligned run out", "d_run_out", run=o.g["run"].ptr(4), cap=cap - 1)
        refused("misaligned rank out", "d_rank_out", rank=o.g["rank"].ptr(8), cap=cap - 2)
        refused("misaligned values out", "d_vals_out", vout=o.g["vals"].ptr(8), cap=cap - 1)
        refused("misaligned count word", "d_num_out", num=o.count.ptr(4))
        refused("misaligned work", "d_work", work=o.work.ptr(8), work_bytes=wb - 8)
        refused("run out is the counts", "d_run_out", "d_counts_in", run=pc.ptr(), cap=n)
        refused("values out overlaps values in", "d_vals_out", "d_vals_in", vout=pv.ptr(16), cap=n - 16)
        refused("rank out overlaps run out", "d_run_out", "d_rank_out", rank=o.g["run"].ptr(16), cap=cap - 4)
        refused("the count word lies in the counts", "d_num_out", "d_counts_in", num=pc.ptr(8))
        refused("the work buffer is the values", "d_work", "d_vals_in", work=pv.ptr(), work_bytes=8 * n)
        refused("num_runs + cap beyond the limit", "num_runs + cap", cap=LIMIT + 1 - n)
        refused("num_runs beyond size_t's half", "num_runs + cap", n=(1 << 64) - 1)
        msg = refused("work one byte short", "adlhip_expand_scratch_bytes", work_bytes=wb - 1)
        assert str(wb) in msg
        o.untouched()
        assert pc.unchanged() and pv.unchanged()
        assert dev.getParam("debug.idle_dirty") == 0
        run, rank, vout, total = expand_oracle(counts, vals)
        assert call_expand(dev, pc.ptr(), n, 8, pv.ptr(), cap, o) == 0, lib_err()
        o.check({"run": run, "rank": rank, "vals": vout}, total, "after the refusals")
    finally:
        for x in (pc, pv, o):
            x.release()


# ---------------------------------------------------------------------------------------------
# the Pprims mirror
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    p = Pprims()
    na, nb = T + 11, T // 2 + 1
    rng = np.random.default_rng(66)
    bufs = []

    def dbuf(arr):
        buf = Buffer(dev, max(arr.size, 1), arr.dtype)
        if arr.size:
            buf.write(arr)
        bufs.append(buf)
        return buf

    try:
        for kname, descending in (("f32", False), ("i64", True)):
            order = DESC if descending else ASC
            udt, kdt = BY_NAME[kname][3], BY_NAME[kname][2]
            a, b = (sort_bits(rng.integers(0, 700, size=m).astype(udt) << udt(20), kname, order) for m in (na, nb))
            ba, bb = dbuf(a.view(kdt)), dbuf(b.view(kdt))
            for name in KINDS:
                ia, ib, total = join_oracle(a, b, kname, KINDS.index(name), order)
                r = p.joinSorted(dev, name, ba, bb, na, nb, descending=descending)                # the counting call
                bufs.append(r.count)
                assert r.indexA is None and r.indexB is None and int(r.count.toHost()[0]) == total
                r = p.joinSorted(dev, name, ba, bb, na, nb, cap=total + 3, indexA=True, indexB=True, descending=descending)
                bufs.extend([r.indexA, r.indexB, r.count])
                assert int(r.count.toHost()[0]) == total
                assert np.array_equal(r.indexA.toHost()[:total], ia) and np.array_equal(r.indexB.toHost()[:total], ib)
                mine, cnt = Buffer(dev, max(total // 2, 1), np.uint32), Buffer(dev, 1, np.uint64)
                bufs.extend([mine, cnt])
                if total // 2:
                    r = p.joinSorted(dev, name, ba, bb, na, nb, cap=total // 2, indexB=mine, countOut=cnt, descending=descending)
                    assert r.indexA is None and r.indexB is mine and r.count is cnt
                    assert int(cnt.toHost()[0]) == total and np.array_equal(mine.toHost()[:total // 2], ib[:total // 2])
            assert np.array_equal(ba.toHost().view(udt), a) and np.array_equal(bb.toHost().view(udt), b)
        counts = rng.integers(0, 4, size=na).astype(np.uint32)
        vals = random_bits(np.uint64, na, rng)
        run, rank, vout, total = expand_oracle(counts, vals)
        bc, bv = dbuf(counts), dbuf(vals.view(np.float64))
        r = p.expandRuns(dev, bc, na)
        bufs.append(r.count)
        assert r.run is None and int(r.count.toHost()[0]) == total
        out = Buffer(dev, total, np.float64)
        bufs.append(out)
        r = p.expandRuns(dev, bc, na, cap=total, values=bv, runOut=True, rankOut=True, valuesOut=out)
        bufs.extend([r.run, r.rank, r.count])
        assert r.values is out and int(r.count.toHost()[0]) == total
        assert np.array_equal(r.run.toHost(), run) and np.array_equal(r.rank.toHost(), rank) and np.array_equal(out.toHost().view(np.uint64), vout)
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for buf in bufs:
            buf.release()
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


_TORCH_KNAME = {"int32": "i32", "int64": "i64", "float32": "f32", "float64": "f64"}


def _torch_values(dtype, n, seed, span=40):
    """no NaN, no -0 (no zero at all among the floats)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-span, span, (n,), dtype=torch.int64, device="cuda", generator=g)
    if dtype.is_floating_point:
        return torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25
    return t.to(dtype)


def _bits(t):
    x = t.cpu().numpy()
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _signed(ib):
    """the oracle's positions in B as TorchSorter.join returns them: int64, -1 for NONE"""
    x = ib.astype(np.int64)
    x[ib == NONE] = -1
    return x


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_join_matches_the_oracle(sorter, dtype_name, descending):
    dt = getattr(torch, dtype_name)
    kname = _TORCH_KNAME[dtype_name]
    order = DESC if descending else ASC
    for na, nb, span in ((T + 7, T // 2 + 1, 300), (5, 0, 3), (0, 4, 3), (1, 1, 1), (0, 0, 1)):
        a = torch.sort(_torch_values(dt, na, 21 + na, span), descending=descending, stable=True).values
        b = torch.sort(_torch_values(dt, nb, 22 + nb, span), descending=descending, stable=True).values
        keep = [x.clone() for x in (a, b)]
        for kind, how in enumerate(KINDS):
            ia, ib, total = join_oracle(_bits(a), _bits(b), kname, kind, order)
            got = sorter.join(a, b, how=how, descending=descending)
            if how in ("semi", "anti"):
                assert isinstance(got, torch.Tensor)
                got = (got,)
            else:
                assert len(got) == 2 and got[1].dtype == torch.int64 and np.array_equal(got[1].cpu().numpy(), _signed(ib)), how
            assert got[0].dtype == torch.int64 and got[0].numel() == total and np.array_equal(got[0].cpu().numpy(), ia.astype(np.int64)), how
        for x, y in zip((a, b), keep):
            assert torch.equal(x, y), "an input was changed"


@pytest.mark.parametrize("dtype_name", ["int32", "int64"])
def test_torch_sorter_join_matches_intersect_on_duplicate_free_inputs(sorter, dtype_name):
    dt = getattr(torch, dtype_name)
    rng = np.random.default_rng(12)
    pool = rng.permutation(np.arange(-3000, 3000))
    x, y = np.sort(pool[:T + 300]), np.sort(pool[T:2 * T + 900])          # 300 shared
    a, b = torch.tensor(x, dtype=dt, device="cuda"), torch.tensor(y, dtype=dt, device="cuda")
    ia, ib = sorter.join(a, b)
    keys, idx = sorter.intersect(a, b, return_indices=True)
    assert ia.numel() == 300 and torch.equal(ia, idx) and torch.equal(a[ia], keys) and torch.equal(b[ib], keys)
    assert torch.equal(sorter.join(a, b, how="semi"), idx)
    _, rest = sorter.difference(a, b, return_indices=True)
    assert torch.equal(sorter.join(a, b, how="anti"), rest)
    la, lb = sorter.join(a.flip(0), b.flip(0), how="left", descending=True)
    assert torch.equal(la, torch.arange(a.numel(), device="cuda")) and int((lb >= 0).sum()) == 300
    assert torch.equal(b.flip(0)[lb[lb >= 0]], a.flip(0)[la[lb >= 0]])


def test_torch_sorter_join_on_offset_views_makes_no_copy(sorter, monkeypatch):
    t = torch.sort(_torch_values(torch.float32, T + 2, 31, 200)).values
    u = torch.sort(_torch_values(torch.int64, T + 4, 32, 200)).values
    seen = []
    real = sorter.pprims.joinSorted
    monkeypatch.setattr(sorter.pprims, "joinSorted", lambda dev, kind, a, b, *r, **k: (seen.append((a.m_ptr, b.m_ptr)), real(dev, kind, a, b, *r, **k))[1])
    for x, y, kname in ((t[1:], t[3:T], "f32"), (u[1:], u[T // 2 + 1:], "i64")):
        assert x.data_ptr() % 16 and y.data_ptr() % 16
        ia, ib, total = join_oracle(_bits(x), _bits(y), kname, INNER, ASC)
        ga, gb = sorter.join(x, y)
        assert np.array_equal(ga.cpu().numpy(), ia.astype(np.int64)) and np.array_equal(gb.cpu().numpy(), _signed(ib))
        assert len(seen) >= 2 and all(s == (x.data_ptr(), y.data_ptr()) for s in seen[-2:]), "a view was copied"
    ga, gb = sorter.join(t[::2], t[1::2])                      # strided views are copied, and joined all the same
    ia, ib, _ = join_oracle(_bits(t[::2]), _bits(t[1::2]), "f32", INNER, ASC)
    assert np.array_equal(ga.cpu().numpy(), ia.astype(np.int64)) and np.array_equal(gb.cpu().numpy(), _signed(ib))


def test_torch_sorter_join_refuses_what_it_cannot_take(sorter):
    a = torch.arange(6, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        sorter.join(a, a, how="outer")
    with pytest.raises(TypeError):
        sorter.join(a, a.to(torch.int64))
    with pytest.raises(TypeError):
        sorter.join(a.to(torch.float16), a.to(torch.float16))
    with pytest.raises(ValueError):
        sorter.join(a.reshape(2, 3), a)
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        with pytest.raises(RuntimeError):
            sorter.join(a, a)
    ia, ib = sorter.join(a, a[2:])
    assert ia.tolist() == [2, 3, 4, 5] and ib.tolist() == [0, 1, 2, 3]
    ia, ib = sorter.join(a, a[2:], how="left")
    assert ia.tolist() == [0, 1, 2, 3, 4, 5] and ib.tolist() == [-1, -1, 0, 1, 2, 3]


@pytest.mark.parametrize("dtype_name", ["int32", "int64", "float32", "float64"])
def test_torch_sorter_repeat_interleave_matches_torch(sorter, dtype_name, monkeypatch):
    dt = getattr(torch, dtype_name)
    g = torch.Generator(device="cuda").manual_seed(5)
    for n, top in ((T + 7, 4), (1, 3), (0, 3), (3 * T, 2), (300, 40)):
        v = _torch_values(dt, n, 60 + n, 1000)
        for rdt in (torch.int64, torch.int32):
            reps = torch.randint(0, top, (n,), dtype=rdt, device="cuda", generator=g)
            want = torch.repeat_interleave(v, reps)
            got = sorter.repeat_interleave(v, reps)
            assert got.dtype == dt and torch.equal(got, want)
            assert torch.equal(sorter.repeat_interleave(v, reps, output_size=want.numel()), want)
        assert torch.equal(sorter.repeat_interleave(v, 3), torch.repeat_interleave(v, 3))
        if n > 4:
            assert torch.equal(sorter.repeat_interleave(v[1:], reps[1:]), torch.repeat_interleave(v[1:], reps[1:]))     # offset views
    # with output_size nothing reaches the host: no counting call, no read of the count
    v, reps = _torch_values(dt, 100, 1, 9), torch.full((100,), 2, dtype=torch.int64, device="cuda")
    calls = []
    real = sorter.pprims.expandRuns
    monkeypatch.setattr(sorter.pprims, "expandRuns", lambda *a, **k: (calls.append(k.get("cap", 0)), real(*a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a host read"))
    assert sorter.repeat_interleave(v, reps, output_size=200).numel() == 200 and calls == [200]
    with pytest.raises(TypeError):
        sorter.repeat_interleave(v.to(torch.float16), reps)
    with pytest.raises(TypeError):
        sorter.repeat_interleave(v, reps.to(torch.float32))
    with pytest.raises(ValueError):
        sorter.repeat_interleave(v, reps[:50])


# ---------------------------------------------------------------------------------------------
# the top of the range
# ---------------------------------------------------------------------------------------------
def test_join_positions_past_2p31_come_back_unsigned_and_exact():
    """A = the numbers 0 .. 2^31 + 12344 as u32 keys, B = 4099 even numbers from 2^31 + 1000 on: every key of B is in A, at a position
    past 2^31.  Inner join: row j is (B[j], j).  Inputs generated and rows verified on the device, as tests/test_gpu_large_n.py does."""
    na, nb, cap = (1 << 31) + 12345, 4099, 4099 + 100
    first = (1 << 31) + 1000
    old = L.CHUNK
    L.CHUNK = 1 << 26
    lib = _lib.load()
    dev = DeviceUtils.allocate(stream=torch.cuda.current_stream().cuda_stream)
    try:
        wb = ctypes.c_size_t()
        assert lib.adlhip_join_scratch_bytes(dev._h, 0, na, nb, cap, ctypes.byref(wb)) == 0, lib_err()
        a = L.fill(torch.empty(na, dtype=torch.int32, device="cuda"), lambda i: i)
        b = L.fill(torch.empty(nb, dtype=torch.int32, device="cuda"), lambda j: first + 2 * j)
        guard = 1024
        ia = torch.full((cap + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ib = torch.full((cap + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        num = torch.full((1 + guard,), -1, dtype=torch.int64, device="cuda")
        work = torch.full((wb.value + 4096,), 0xA7, dtype=torch.uint8, device="cuda")
        P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        for kind, rows in ((INNER, nb), (SEMI, nb)):
            rc = lib.adlhip_join_sorted_typed(dev._h, 0, ASC, kind, P(a), na, P(b), nb, cap, P(ia), P(ib), P(num), P(work), wb.value)
            assert rc == 0, lib_err()
            torch.cuda.synchronize()
            assert lib.adlhip_fault_check(dev._h) == 0, lib_err()
            assert int(num[0].item()) == rows
            j = torch.arange(nb, device="cuda", dtype=torch.int64)
            assert torch.equal(L.from_u32(ia[:nb]), first + 2 * j), "positions in A past 2^31"
            assert torch.equal(L.from_u32(ib[:nb]), j)
            assert bool((ia[nb:] == 0x5A5A5A5A).all()) and bool((ib[nb:] == 0x5A5A5A5A).all()), "written behind the rows"
            assert bool((num[1:] == -1).all()) and bool((work[wb.value:] == 0xA7).all()), "written behind the count word or the work buffer"
        L.check_equal(a, lambda i: i, na, "a afterwards")
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        L.CHUNK = old
        a = b = ia = ib = num = work = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        DeviceUtils.deallocate(dev)
