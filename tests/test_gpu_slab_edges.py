"""Slab and tile edges of the large and mid-size sorts (run with `-m gpu` on the MI355X box).

The large sort (cursor, stable and hybrid forms) and the mid-size sort place keys in fixed-capacity regions whose sizes the host
computes from n: pass-1 bucket slabs (or per-chain sub-slabs), segment slabs and the finish's tile.  A run that does not fit
raises a flag and the safety net re-sorts the untouched input -- correct, 3-4x slower, and visible only in "stat.net_runs".
Random keys stay far below those edges, so here every targeted region is filled to exactly cap - 1, cap and cap + 1 keys.

A Python mirror of the host's capacities (tests/large_plan.py and below, with the source it restates) predicts each run's outcome: the result is
bit-exact against the oracle, the safety net runs exactly when some region overflows, the kernels that ran are the form and
finish the case claims, and the device fault word stays clean.
"""
import ctypes
import math

import numpy as np
import pytest

import oracle
from oclradixsort_amd import DeviceUtils, Buffer, _lib
from oclradixsort_amd._lib import check

from large_plan import KV32, LEAN_PCT, MI, SOA32, U32, U64, large_sort_form, msd2_layout, msd2s_layout


# ---------------------------------------------------------------------------------------------
# mirror of the host's capacities: the large sort's is tests/large_plan.py (oclradixsort_amd/csrc/large_plan.hpp)
# ---------------------------------------------------------------------------------------------
def mid_stride(n):
    """adlhip.hip mid_layout().stride: the mid-size sort's bucket slab (= its LDS tile; adlhip.hip mid_sort uses the same cap)"""
    return 4096 if n <= (512 << 10) else 8192 if n <= MI else 16384


def finish_names(kind, form, w, tier_b, whole=True):
    """The finish's launches (adlhip.hip launch_large_finish, default knobs): the workgroup-per-segment finish for whole u32
    keys with 65536 segments and a tile of 3072 and more (or beyond 5120), the binning finish + its listed hand-over for whole
    u64 keys (large_plan.hpp use_bin_finish: n >= 24 Mi, or any n with a narrow second digit), else the wave LSD finish
    (wave_finish16_kernel for the 16-bit second slab, 1280 / 1536 / 2560)."""
    if kind == U32:
        return {"segment_sort_wg_u32"} if (tier_b > 5120 or (whole and w == 8 and tier_b >= 3072)) else {"segment_sort_wave_u32"}
    if kind == U64 and whole:
        return {"segment_sort_bin_u64", "segment_sort_listed_e64"}
    return {"segment_sort_wave_e64"}


def large_names(kind, form, w, tier_b, whole=True):
    suffix = {U32: "u32", U64: "u64", KV32: "kv32", SOA32: "soa"}[kind]
    if form == "cursor":
        names = {"msd2_sample", "msd2_pass1_" + suffix, "msd2_pass2_" + suffix, "msd2_offsets"}
    else:
        second = ("msd2h_pass2_" if form == "hybrid" else "msd2s_pass2_") + suffix
        names = {"msd2s_prep", "msd2s_pass1_" + suffix, second, "msd2s_offsets"}
    return names | finish_names(kind, form, w, tier_b, whole)


def test_mirror_matches_the_capacities_read_from_the_code():
    """The mirror restates the host's arithmetic; the values in the test plan were read from the code.  (The GPU cases below are
    what checks both against the library: a capacity one step off turns a cap / cap + 1 pair around.)"""
    for n_mi, sa, sa_lean, w, sb, tb in ((3, 22528, 17920, 4, 1216, 1536), (24, 151552, 114240, 8, 640, 1280),
                                         (64, 397312, 297728, 8, 1536, 1536)):
        L = msd2_layout(n_mi * MI, 4)
        assert (L["stride_a"], msd2_layout(n_mi * MI, 4, LEAN_PCT)["stride_a"], L["seg_shift"], L["stride_b"], L["tier_b"]) == \
            (sa, sa_lean, w, sb, tb), n_mi
    for n_mi, sb, tb in ((100, 2432, 2560), (150, 3072, 3072), (200, 4096, 4096), (260, 5120, 5120)):
        L = msd2_layout(n_mi * MI, 4)
        assert (L["seg_shift"], L["stride_b"], L["tier_b"]) == (8, sb, tb), n_mi
    for n_mi, sa, sa_lean, w, sb, sb_lean in ((64, 25664, 17472, 8, 1536, 1280), (5, 2304, 1664, 5, 1024, 896)):
        L, Ll = msd2s_layout(n_mi * MI), msd2s_layout(n_mi * MI, lean=True)
        assert (L["stride_a"], Ll["stride_a"], L["seg_shift"], L["stride_b"], Ll["stride_b"], L["tier_b"]) == \
            (sa, sa_lean, w, sb, sb_lean, 1536), n_mi
    L = msd2_layout(30 * MI, 8)
    assert (L["stride_a"], L["seg_shift"], L["stride_b"], L["tier_b"]) == (188416, 7, 1472, 1536)
    # a full pass-1 bucket fits its segment slabs (stride_a <= 2^w stride_b) at 12 (exactly), 24, 32 and 100 Mi keys, not at 3,
    # 5, 64 and 150 Mi; at lean head-room it does at 64 Mi
    for n_mi, fits in ((3, False), (5, False), (12, True), (24, True), (32, True), (64, False), (100, True), (150, False)):
        L = msd2_layout(n_mi * MI, 4)
        assert (L["stride_a"] <= (L["stride_b"] << L["seg_shift"])) == fits, n_mi
    L = msd2_layout(12 * MI, 4)
    assert L["stride_a"] == L["stride_b"] << L["seg_shift"] == 77824
    L = msd2_layout(64 * MI, 4, LEAN_PCT)
    assert L["stride_a"] <= L["stride_b"] << L["seg_shift"]
    assert [mid_stride(n) for n in ((512 << 10), (512 << 10) + 1, MI, MI + 1, 2 * MI)] == [4096, 8192, 8192, 16384, 16384]
    assert large_sort_form(U32, 64 * MI, 32, 1) == "cursor" and large_sort_form(U32, 200 * MI, 32, 1) == "hybrid"
    assert large_sort_form(U64, 64 * MI, 64, 1) == "stable" and large_sort_form(KV32, 64 * MI, 32, 4) == "stable"
    assert large_sort_form(U32, 5 * MI, 24, 4) == "stable" and large_sort_form(KV32, 64 * MI, 32, 3, rank=0) == "stable"
    assert large_sort_form(U32, 5 * MI, 32, 1, rank=0) is None
    assert finish_names(U32, "cursor", 8, 4096) == {"segment_sort_wg_u32"} and finish_names(U32, "cursor", 4, 1536) == {"segment_sort_wave_u32"}


# ---------------------------------------------------------------------------------------------
# keys with exact counts per segment (first digit, second digit)
# ---------------------------------------------------------------------------------------------
def _mix(n, rng):
    """A well-scattered permutation of range(n), much cheaper than rng.permutation at 64 Mi: a multiplicative (Weyl) step that
    spreads every run over the whole array, then 64-element rows shuffled and their columns permuted."""
    a = int(n * 0.6180339887) | 1
    while math.gcd(a, n) != 1:
        a += 2
    idx = (np.arange(n, dtype=np.int64) * a) % n
    m = n - n % 64
    rows = idx[:m].reshape(-1, 64)
    rng.shuffle(rows)
    idx[:m] = rows[:, rng.permutation(64)].ravel()
    return idx


class Keys:
    """Keys whose segments -- slot (first digit << w) | second digit, the digits at [top - 8, top) and [top - 8 - w, top - 8)
    -- hold exactly counts[slot] keys; random below, zero above top (bits above top are part of the key and must be the
    same in every key, msd2_placement), or random there when the sort looks at the low `top` bits only (noise_above).
    Full segments hold low-16 values 0x0000 and 0xFFFF (a tile's last row unpadded is where a slip shows); `repeats` repeats
    keys inside them (pairs: stability); `hard` segments keep the top 16 of their low bits constant (the binning finish cannot
    bin them and hands them to its listed LSD form)."""

    def __init__(self, n, top, w, key_bits, counts, seed, full=(), hard=(), repeats=False, noise_above=False):
        counts = np.asarray(counts, dtype=np.int64)
        assert counts.size == 256 << w and counts.sum() == n and counts.min() >= 0
        self.n, self.top, self.w, self.key_bits = n, top, w, key_bits
        self.lb = top - 8 - w
        rng = np.random.default_rng(seed)
        dt = np.uint32 if key_bits == 32 else np.uint64
        lb = self.lb
        keys = np.repeat(np.arange(counts.size, dtype=dt), counts) << dt(lb)
        if key_bits == 32:
            keys |= rng.integers(0, 1 << lb, n, dtype=np.uint32)
        else:
            keys |= rng.bit_generator.random_raw(n) >> np.uint64(64 - lb)
        starts = np.concatenate(([0], np.cumsum(counts)))
        for s in hard:
            seg = keys[starts[s]:starts[s + 1]]
            seg &= ~dt(((1 << 16) - 1) << (lb - 16))
            seg |= dt(0x5a5a << (lb - 16))
        for s in full:
            seg = keys[starts[s]:starts[s + 1]]
            base = dt(s << lb)
            seg[0], seg[1] = base, base | dt((1 << lb) - 1)
            if repeats:
                r = seg[8::8]
                r[:] = seg[7::8][:r.size]
        if noise_above and top < key_bits:
            keys |= rng.integers(0, 1 << (key_bits - top), n, dtype=dt) << dt(top)
        self.keys = keys[_mix(n, rng)]
        self._sorted = None

    def slots(self, keys=None):
        k = self.keys if keys is None else keys
        return ((k >> type(k[0])(self.lb)) & type(k[0])((1 << (8 + self.w)) - 1)).astype(np.int64)

    def move(self, keys, src, dst, nth=0):
        """keys with one key of slot src moved to slot dst (its other bits kept): n stays, one count changes each way"""
        out = keys.copy()
        i = np.flatnonzero(self.slots(keys) == src)[nth]
        dt = type(keys[0])
        mask = dt(((1 << (8 + self.w)) - 1) << self.lb)
        out[i] = (out[i] & ~mask) | dt(dst << self.lb)
        return Moved(out, keys, keys[i], out[i])

    def sorted(self):
        """the oracle's sort of self.keys (whole keys), once"""
        if self._sorted is None:
            self._sorted = oracle.sort_u32(self.keys) if self.key_bits == 32 else oracle.sort_u64(self.keys)
        return self._sorted


class Moved:
    """keys that differ from `base` in one key, old -> new"""

    def __init__(self, keys, base, old, new):
        self.keys, self.base, self.old, self.new = keys, base, old, new


def _one_key_replaced(s, old, new):
    """the sorted array s with one copy of old replaced by new (whole keys: equal keys are indistinguishable)"""
    i = int(np.searchsorted(s, old))
    assert s[i] == old
    t = np.delete(s, i)
    return np.insert(t, int(np.searchsorted(t, new)), new)


def even_counts(n, slots, targets=None, keep_buckets=(), w=8):
    """n keys over `slots` segments as evenly as possible; targets {slot: count} exactly; the difference taken from (or given
    to) the other segments, outside the buckets in keep_buckets, evenly"""
    c = np.full(slots, n // slots, dtype=np.int64)
    c[: n % slots] += 1
    targets = targets or {}
    for s, v in targets.items():
        c[s] = v
    fixed = np.zeros(slots, dtype=bool)
    fixed[list(targets)] = True
    for b in keep_buckets:
        fixed[b << w:(b + 1) << w] = True
    donors = np.flatnonzero(~fixed)
    q, r = divmod(int(c.sum()) - n, donors.size)
    c[donors] -= q
    c[donors[:r]] -= 1
    assert c.sum() == n and c.min() >= 0
    return c


def bucket_counts(total, w):
    """one bucket's `total` keys over its 2^w segments as evenly as possible"""
    k = 1 << w
    c = np.full(k, total // k, dtype=np.int64)
    c[: total % k] += 1
    return c


def overflows(K, keys, form, L):
    """The mirror's prediction from the keys themselves: does any run exceed its slab?  cursor: a bucket beyond stride_a or a
    segment beyond stride_b; stable / hybrid: the keys of one bucket in one chain's input slice beyond stride_a, or a segment
    beyond stride_b."""
    s = K.slots(keys)
    seg = np.bincount(s, minlength=256 << K.w)
    over = int(seg.max()) > L["stride_b"]
    b = s >> K.w
    if form == "cursor":
        over |= int(np.bincount(b, minlength=256).max()) > L["stride_a"]
    else:
        for p in range(L["pieces"]):
            part = b[p * L["slice"]:(p + 1) * L["slice"]]
            if part.size:
                over |= int(np.bincount(part, minlength=256).max()) > L["stride_a"]
    return int(over), seg


# ---------------------------------------------------------------------------------------------
# running one sort through the ABI
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    DeviceUtils.deallocate(d)


def _defaults(d):
    for name, value in (("sort.algo", -1), ("sort.digit_bits", 8), ("sort.tile", -1), ("sort.rank", 1), ("sort.msd2", 1),
                        ("sort.mid", 1), ("sort.dict", 1), ("sort.binfinish", 1), ("sort.persist", 1)):
        d.setParam(name, value)


@pytest.fixture(autouse=True)
def _knobs(request):
    if "dev" in request.fixturenames:
        d = request.getfixturevalue("dev")
        _defaults(d)
        yield
        _defaults(d)
    else:
        yield


def _sort(d, kind, host, bits, level=1, vals=None):
    """One sort of `host` through the C ABI with the work buffer of scratch level `level`; returns (result, profile, nets run)."""
    lib = _lib.load()
    n = host.size
    tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.adlhip_radix_sort_scratch_bytes_for(d._h, kind, n, bits, level, ctypes.byref(tb), ctypes.byref(wb)), "scratch")
    dt = np.uint32 if kind in (U32, SOA32) else np.uint64
    bufs = [Buffer(d, n, dt), Buffer(d, max(n, tb.value // np.dtype(dt).itemsize), dt), Buffer(d, wb.value, np.uint8)]
    if kind == SOA32:
        bufs += [Buffer(d, n, np.uint32), Buffer(d, n, np.uint32)]
    try:
        bufs[0].write(host)
        if kind == SOA32:
            bufs[3].write(vals)
        runs0 = d.getParam("stat.net_runs")
        d.toggleProfiling(True)
        d.profile(reset=True)
        try:
            data, tmp, work = (b.ptr() for b in bufs[:3])
            if kind == U32:
                rc = lib.adlhip_radix_sort_u32(d._h, data, tmp, work, wb.value, n, bits)
            elif kind == KV32:
                rc = lib.adlhip_radix_sort_kv32(d._h, data, tmp, work, wb.value, n, bits)
            elif kind == U64:
                rc = lib.adlhip_radix_sort_u64(d._h, data, tmp, work, wb.value, n, bits)
            else:
                rc = lib.adlhip_radix_sort_soa32(d._h, data, bufs[3].ptr(), tmp, bufs[4].ptr(), work, wb.value, n, bits)
            check(rc, "sort")
            out = bufs[0].toHost()
            if kind == SOA32:
                out = (out, bufs[3].toHost())
        finally:
            prof = d.profile(reset=True)
            d.toggleProfiling(False)
        return out, prof, d.getParam("stat.net_runs") - runs0
    finally:
        for b in bufs:
            b.release()


def _expected(kind, keys, bits, vals=None):
    if kind == SOA32:
        return oracle.sort_soa(keys, vals, bits)
    if kind == U32:
        return oracle.sort_u32(keys) if bits == 32 else oracle.sort_u32_bits(keys, bits)
    if kind == U64:
        return oracle.sort_u64(keys) if bits == 64 else oracle.sort_e64_bits(keys, bits)
    return oracle.sort_kv32(keys) if bits == 32 else oracle.sort_e64_bits(keys, bits)


def _elements(kind, keys):
    """what the sort gets: keys, or {key, value = input index} pairs (AoS), or (keys, indices) (SoA)"""
    if kind == KV32:
        return keys.astype(np.uint64) | (np.arange(keys.size, dtype=np.uint64) << np.uint64(32))
    return keys


def _run_case(d, name, kind, K, keys, bits, form, L, want_net, level=1):
    """sort, then assert: bit-exact vs the oracle; the mirror's prediction is the one the case was built for; the safety net ran
    exactly when the mirror says a run overflows; the kernels of the claimed form and finish; a clean fault word."""
    whole = bits == (64 if kind == U64 else 32)
    moved = keys if isinstance(keys, Moved) else None
    keys = moved.keys if moved else keys
    pred, _ = overflows(K, keys, form, L)
    assert pred == want_net, (name, "the keys were not built as the case claims")
    vals = np.arange(keys.size, dtype=np.uint32) if kind == SOA32 else None
    host = _elements(kind, keys)
    got, prof, net = _sort(d, kind, host, bits, level, vals)
    if kind in (U32, U64) and whole and (keys is K.keys or (moved and moved.base is K.keys)):
        # whole keys: the oracle's sort of the case's base input, with the one moved key taken out and put back in
        want = K.sorted() if not moved else _one_key_replaced(K.sorted(), moved.old, moved.new)
    else:
        want = _expected(kind, host, bits, vals)
    if kind == SOA32:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    else:
        assert np.array_equal(got, want), name
    assert net == pred, (name, "safety net runs", net, "mirror predicts", pred)
    assert set(prof) == large_names(kind, form, L["seg_shift"], L["tier_b"], whole), (name, sorted(prof))
    d.checkFault()


def _triple(d, tag, kind, K, keys_cap, bits, form, L, target, donor, nets, level=1):
    """cap - 1, cap and cap + 1 keys in slot `target` (one key moved to / from slot `donor`); nets = the safety net expected for
    each"""
    variants = (("cap-1", K.move(keys_cap, target, donor)), ("cap", keys_cap), ("cap+1", K.move(keys_cap, donor, target)))
    for (label, keys), net in zip(variants, nets):
        _run_case(d, "%s %s" % (tag, label), kind, K, keys, bits, form, L, net, level)


# ---------------------------------------------------------------------------------------------
# cursor form ("sort.msd2" = 4): segment slabs at their edge
# ---------------------------------------------------------------------------------------------
CURSOR_SEGMENTS = [
    # (n, key kind, top, seed): narrow second digit (3 Mi, w = 4, wave LSD finish 1536, slab 1216), full second digit (24 Mi:
    # slab 640 in the 1280 tile of wave_finish16; 64 Mi: slab = tile = 1536, full tiles without padding), keys shifted down
    # (top 29: the digits sit lower), u64 keys with the binning finish (30 Mi, w = 7, slab 1472)
    pytest.param(3 * MI + 17, U32, 32, 1, id="u32-3Mi-w4"),
    pytest.param(3 * MI + 17, U32, 27, 2, id="u32-3Mi-w4-top27"),
    pytest.param(24 * MI + 5, U32, 32, 3, id="u32-24Mi-tile1280"),
    pytest.param(24 * MI + 5, U32, 29, 4, id="u32-24Mi-top29"),
    pytest.param(64 * MI, U32, 32, 5, id="u32-64Mi-tile1536"),
    pytest.param(30 * MI + 3, U64, 64, 6, id="u64-30Mi-binfinish"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind,top,seed", CURSOR_SEGMENTS)
def test_cursor_segment_slab_edges(dev, n, kind, top, seed):
    eb = 4 if kind == U32 else 8
    L = msd2_layout(n, eb)
    w, cap = L["seg_shift"], L["stride_b"]
    dev.setParam("sort.msd2", 4)
    assert large_sort_form(kind, n, 8 * eb, 4) == "cursor"
    slots = 256 << w
    # full segments: two in bucket 0 (neighbouring slabs), one in the middle, the last slot of all; u64: one more whose keys
    # cannot be binned (the listed hand-over gets a full segment)
    full = [0, 1, slots // 2 + 3, slots - 1]
    hard = [slots // 4 + 5] if kind == U64 else []
    donor = slots // 3
    counts = even_counts(n, slots, {s: cap for s in full + hard})
    K = Keys(n, top, w, 8 * eb, counts, seed, full=full + hard, hard=hard)
    _triple(dev, "cursor n=%d slab %d tile %d" % (n, cap, L["tier_b"]), kind, K, K.keys, 8 * eb, "cursor", L,
            target=slots // 2 + 3, donor=donor, nets=(0, 0, 1))
    if hard:   # the hard segment itself over its slab
        _run_case(dev, "hard segment cap+1", kind, K, K.move(K.keys, donor, hard[0]), 8 * eb, "cursor", L, 1)


@pytest.mark.gpu
def test_cursor_workgroup_finish_tile_4096(dev):
    """~200 Mi u32 keys: segment slab = tile = 4096, the workgroup-per-segment finish (256 x 16) with full tiles."""
    n = 200 * MI
    L = msd2_layout(n, 4)
    assert (L["seg_shift"], L["stride_b"], L["tier_b"]) == (8, 4096, 4096)
    dev.setParam("sort.msd2", 4)
    full = [7, 8, 40000, 65535]
    K = Keys(n, 32, 8, 32, even_counts(n, 65536, {s: 4096 for s in full}), 11, full=full)
    _triple(dev, "cursor 200 Mi tile 4096", U32, K, K.keys, 32, "cursor", L, target=40000, donor=12345, nets=(0, 0, 1))


# ---------------------------------------------------------------------------------------------
# cursor form: pass-1 bucket slabs at their edge
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_mi", [3, 5, 12, 24, 32, 64])
def test_cursor_bucket_slab_edges(dev, n_mi):
    """One bucket with stride_a - 1, stride_a, stride_a + 1 keys, spread evenly over its segments.  Where 2^w stride_b >=
    stride_a (12 Mi: equal, both regions exactly full at once; 24, 32 Mi) a full bucket fits and only cap + 1 goes to the net;
    where it is smaller (3, 5, 64 Mi) the full bucket must overflow its segment slabs, and the mirror predicts the net for all
    three."""
    n = n_mi * MI
    L = msd2_layout(n, 4)
    w, cap = L["seg_shift"], L["stride_a"]
    fits = cap <= L["stride_b"] << w
    dev.setParam("sort.msd2", 4)
    b = 77
    per = bucket_counts(cap, w)
    counts = even_counts(n, 256 << w, {(b << w) + i: int(c) for i, c in enumerate(per)}, keep_buckets=(b,), w=w)
    K = Keys(n, 32, w, 32, counts, 100 + n_mi, full=[(b << w) + int(np.argmax(per))])
    # cap - 1: a key leaves the bucket's fullest segment; cap + 1: a key joins its least full one
    lo, hi = (b << w) + int(np.argmin(per)), (b << w) + int(np.argmax(per))
    donor = ((b + 100) << w) + 3
    variants = (("cap-1", K.move(K.keys, hi, donor), 0 if fits else 1), ("cap", K.keys, 0 if fits else 1),
                ("cap+1", K.move(K.keys, donor, lo), 1))
    if n_mi == 12:
        assert cap == L["stride_b"] << w and per.min() == per.max() == L["stride_b"]
    for label, keys, net in variants:
        _run_case(dev, "bucket n=%d Mi stride_a %d %s" % (n_mi, cap, label), U32, K, keys, 32, "cursor", L, net)


# ---------------------------------------------------------------------------------------------
# lean scratch (level 2): 12 % bucket slabs of the cursor form
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lean_cursor_bucket_slab_edge_64mi(dev):
    """64 Mi u32 keys with the level-2 work buffer: the bucket slab is 297728 keys, which its segment slabs hold (256 x 1536), so
    a bucket of exactly that many keys keeps full speed and one more key takes the net."""
    n = 64 * MI
    L = msd2_layout(n, 4, LEAN_PCT)
    w, cap = L["seg_shift"], L["stride_a"]
    assert cap == 297728 and cap <= L["stride_b"] << w
    dev.setParam("sort.msd2", 4)
    b = 200
    per = bucket_counts(cap, w)
    counts = even_counts(n, 65536, {(b << 8) + i: int(c) for i, c in enumerate(per)}, keep_buckets=(b,))
    K = Keys(n, 32, 8, 32, counts, 21)
    donor = (3 << 8) + 9
    variants = (("cap-1", K.move(K.keys, b << 8, donor), 0), ("cap", K.keys, 0), ("cap+1", K.move(K.keys, donor, (b << 8) + 255), 1))
    for label, keys, net in variants:
        _run_case(dev, "lean bucket %s" % label, U32, K, keys, 32, "cursor", L, net, level=2)


# ---------------------------------------------------------------------------------------------
# stable and hybrid forms: per-chain sub-slabs and segment slabs at their edge
# ---------------------------------------------------------------------------------------------
def _fill_chain(K, keys, L, chain, bucket, want):
    """a copy of keys in which chain `chain`'s input slice holds exactly `want` keys of `bucket`: keys of the bucket from other
    slices swap places with other keys of this slice (every segment keeps its count)"""
    out = keys.copy()
    b = K.slots(out) >> K.w
    lo, hi = chain * L["slice"], min((chain + 1) * L["slice"], keys.size)
    inside = np.arange(lo, hi)
    have = int(np.count_nonzero(b[lo:hi] == bucket))
    k = want - have
    assert k >= 0
    take = np.flatnonzero(b == bucket)
    take = take[(take < lo) | (take >= hi)][:k]
    give = inside[b[lo:hi] != bucket][:k]
    assert take.size == give.size == k
    out[take], out[give] = keys[give], keys[take]
    return out


def _stable_case(dev, tag, kind, n, bits, form, L, seed, key_bits=32, level=1, labels=None):
    """Segment edge (full segments, keys repeated inside them, and one of them cap - 1 / cap + 1) and sub-slab edge (one
    (bucket, chain) with exactly stride_a keys of the sub-slab, then one more) in one input.  The digits sit at the top of the
    sorted bits; bits above them (a sort on part of the key) are random."""
    w, sb, sa = L["seg_shift"], L["stride_b"], L["stride_a"]
    slots = 256 << w
    full = [5, slots // 2 + 1, slots - 2]
    bucket, chain = 150, 3
    counts = even_counts(n, slots, {s: sb for s in full})
    K = Keys(n, bits, w, key_bits, counts, seed, full=full, repeats=True, noise_above=bits < key_bits)
    base = _fill_chain(K, K.keys, L, chain, bucket, sa)
    donor = slots // 3 + 7
    cases = [("segment cap-1", lambda: K.move(base, full[1], donor), 0), ("all at cap", lambda: base, 0),
             ("segment cap+1", lambda: K.move(base, donor, full[1]), 1),
             ("sub-slab cap-1", lambda: _fill_chain(K, K.keys, L, chain, bucket, sa - 1), 0),
             ("sub-slab cap+1", lambda: _fill_chain(K, K.keys, L, chain, bucket, sa + 1), 1)]
    for label, keys, net in cases:
        if labels is None or label in labels:
            _run_case(dev, "%s %s" % (tag, label), kind, K, keys(), bits, form, L, net, level)


STABLE_CASES = [
    # (kind, n, sort bits, knob, rank, level, seed): pairs AoS at 64 Mi (sub-slab 25664, slab = tile 1536), the same with ballot
    # ranking (the ballot-ranked finish at 1536), SoA pairs and u64 keys at 5 Mi (w = 5, sub-slab 2304, slab 1024), u32 keys on
    # 24 bits (bits above random: stability shows), the hybrid form at 64 Mi, lean pairs (sub-slab mean + 8 sd, slab mean + 7.5 sd)
    pytest.param(KV32, 64 * MI, 32, 3, 1, 1, 31, id="pairs-64Mi"),
    pytest.param(KV32, 64 * MI, 32, 3, 0, 1, 32, id="pairs-64Mi-rank0"),
    pytest.param(SOA32, 5 * MI + 9, 32, 3, 1, 1, 33, id="soa-5Mi"),
    pytest.param(U64, 5 * MI + 9, 64, 3, 1, 1, 34, id="u64-5Mi"),
    pytest.param(U32, 5 * MI + 9, 24, 3, 1, 1, 35, id="u32-5Mi-bits24"),
    pytest.param(U32, 64 * MI, 32, 5, 1, 1, 36, id="hybrid-64Mi"),
    pytest.param(KV32, 24 * MI + 1, 32, 3, 1, 2, 37, id="pairs-24Mi-lean"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,bits,knob,rank,level,seed", STABLE_CASES)
def test_stable_and_hybrid_slab_edges(dev, kind, n, bits, knob, rank, level, seed):
    key_bits = 64 if kind == U64 else 32
    whole = bits == key_bits
    form = large_sort_form(kind, n, bits, knob, rank)
    assert form == ("hybrid" if knob == 5 else "stable")
    L = msd2s_layout(n, 4 if kind == U32 else 8, kind == U32 and whole, lean=level == 2)
    dev.setParam("sort.msd2", knob)
    dev.setParam("sort.rank", rank)
    _stable_case(dev, "%s n=%d sub-slab %d slab %d tile %d" % (form, n, L["stride_a"], L["stride_b"], L["tier_b"]), kind, n, bits,
                 form, L, seed, key_bits=key_bits, level=level,
                 labels=("all at cap", "segment cap+1") if rank == 0 else None)   # (rank 0: the ballot-ranked finish's full tile)


# ---------------------------------------------------------------------------------------------
# mid-size sort ("sort.mid" = 2 / 3): bucket slabs of 4096 / 8192 / 16384 keys
# ---------------------------------------------------------------------------------------------
def _mid_overflowed(d, form):
    """Whether the last forced mid-size sort on handle d overflowed a bucket: it reports into pinned memory, and the automatic
    choice of the next eligible sort steers by that report (adlhip.hip choose_mid_form) -- a two-launch overflow keeps the
    next u32 sort off the two-launch form, a three-launch overflow keeps the next {key, value} sort (which has no two-launch
    form) off the three-launch form."""
    d.setParam("sort.mid", 1)
    n = 300007
    if form == 2:
        k = oracle.keys_u32(n, seed=5)
        got, prof, _ = _sort(d, U32, k, 32)
        assert np.array_equal(got, oracle.sort_u32(k))
        return set(prof) != {"mid_bucket_scatter_u32", "segment_sort_u32"}
    p = oracle.pairs_kv32(n, seed=5)
    got, prof, _ = _sort(d, KV32, p, 32)
    assert np.array_equal(got, oracle.sort_kv32(p))
    return "mid_prep_e64" not in prof


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(512 << 10) - 3, MI - 5, 2 * MI - 7])
@pytest.mark.parametrize("form", [2, 3])
def test_mid_size_bucket_slab_edges(n, form):
    """One top-byte bucket of exactly the slab (4096 / 8192 / 16384 keys), one less and one more; the others share the rest.
    Each sort runs on a fresh handle, whose next automatic sort shows whether it overflowed."""
    cap = mid_stride(n)
    assert cap == max(4096, 2 * ((n + 255) // 256))   # the three-launch form's bound (adlhip.hip mid_sort) is the same slab
    b = 201
    counts = even_counts(n, 256, {b: cap}, w=0)
    K = Keys(n, 32, 0, 32, counts, 40 + form, full=[b])
    names = {"mid_bucket_scatter_u32", "segment_sort_u32"} if form == 2 else {"mid_prep_u32", "onesweep_u32_8b", "segment_sort_u32"}
    donor = 17
    for label, keys, over in (("cap-1", K.move(K.keys, b, donor).keys, False), ("cap", K.keys, False),
                              ("cap+1", K.move(K.keys, donor, b).keys, True)):
        assert (int(np.bincount(K.slots(keys), minlength=256).max()) > cap) == over
        d = DeviceUtils.allocate()
        try:
            _defaults(d)
            d.setParam("sort.mid", form)
            got, prof, _ = _sort(d, U32, keys, 32)
            assert np.array_equal(got, oracle.sort_u32(keys)), (n, form, label)
            assert set(prof) == names, (n, form, label, sorted(prof))
            assert _mid_overflowed(d, form) == over, (n, form, label)
            d.checkFault()
        finally:
            DeviceUtils.deallocate(d)
