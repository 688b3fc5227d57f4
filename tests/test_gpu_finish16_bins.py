"""The one-pass form of the 16-bit LDS finish (finish16_kernels.hpp, finish16_bins) (run with `-m gpu` on the MI355X box).

Where the finish sorts more than 8 bits, one LDS pass places a segment's keys by the top B bits of what is left to sort, into a
blocked layout (lane l owns 2 RR consecutive positions), and M rounds of odd-even transposition in registers order the keys that
share a bin; M is the segment's largest bin.  A segment whose largest bin holds more than kFinish16MaxRounds keys, or whose keys
all share one bin, takes the two LSD passes instead.  Positions past the segment's end are padded with 0xffff.

Here the keys are built segment by segment -- (segment << 16) | low -- so that chosen segments hold a bin of exactly the limit's
size, one key less and one more, at either end of the key range and in the middle; keys equal to the pad and to zero; bins that
straddle every boundary between two lanes' blocks; and fewer than 16 bits to sort.

Every case: bit-exact against the oracle's sort of the same keys; exactly the five launches of the cursor form with the wave
finish; the safety net has not run; a clean fault word and an idle handle.  Every case must fit its slabs: nothing is skipped.
"""
import ctypes

import numpy as np
import pytest

import oracle
from oclradixsort_amd import Buffer, DeviceUtils, _lib
from oclradixsort_amd._lib import check

MI = 1 << 20
SLOTS = 65536
LAUNCHES = {"msd2_sample", "msd2_pass1_u32", "msd2_pass2_u32", "msd2_offsets", "segment_sort_wave_u32"}
DYN_LOW_BITS = 4   # hybrid_kernels.hpp kDynLowBits: word of the work buffer's first block that holds the bits the finish sorts
BIN_BITS = 9       # finish16_kernels.hpp kFinish16BinBits
MAX_ROUNDS = 24    # finish16_kernels.hpp kFinish16MaxRounds
BIN_SPAN = 1 << (16 - BIN_BITS)   # key values per bin where the finish sorts 16 bits


def _sd(mean):
    sd = 1
    while sd * sd < mean:
        sd += 1
    return sd


def layout(n):
    """adlhip.hip msd2_layout for whole u32 keys with 65536 segments: (pass-1 bucket slab, segment slab, finish tile)"""
    mean = (n + SLOTS - 1) // SLOTS
    need = mean + (15 * _sd(mean) + 1) // 2
    tier = 1280 if need <= 832 else 1536 if need <= 1280 else 2560
    assert need <= 2560
    stride_b = min((max(mean + mean // 2, need) + 8 + 63) // 64 * 64, tier)
    stride_a = (n // 256 + (n // 256) * 50 // 100 + 4096 + 63) // 64 * 64
    return stride_a, stride_b, tier


def counts_with(n, targets):
    """n keys over the 65536 segments as evenly as possible, segment s holding exactly targets[s]"""
    c = np.full(SLOTS, -1, dtype=np.int64)
    for s, v in targets.items():
        c[s] = v
    free = np.flatnonzero(c < 0)
    rest = n - int(c[c >= 0].sum())
    c[free] = rest // free.size
    c[free[: rest % free.size]] += 1
    assert c.sum() == n and c.min() >= 0
    return c


def build(counts, seed, patch=None):
    """(segment << 16) | random low half, counts[s] keys in segment s; patch(low, starts, rng) may rewrite the low halves of
    chosen segments in place; then a stride permutation spreads every segment over the whole input."""
    n = int(counts.sum())
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    starts = np.concatenate(([0], np.cumsum(counts)))
    if patch:
        patch(low, starts, rng)
    keys = (np.repeat(np.arange(SLOTS, dtype=np.uint32), counts) << np.uint32(16)) | low
    rows = 4096
    m = n - n % rows
    keys[:m] = keys[:m].reshape(rows, -1).T.ravel()
    return keys


def assert_fits(keys, n):
    """The CPU check before anything is sent: no bucket beyond its pass-1 slab, no segment beyond its slab."""
    stride_a, stride_b, _ = layout(n)
    seg = np.bincount(keys >> np.uint32(16), minlength=SLOTS)
    assert int(seg.max()) <= stride_b, ("a segment overflows its slab", int(seg.max()), stride_b)
    assert int(seg.reshape(256, 256).sum(axis=1).max()) <= stride_a, "a bucket overflows its pass-1 slab"


def largest_bin(keys, s, bits=16):
    """the largest bin (top BIN_BITS of the `bits` the finish sorts) of segment s"""
    low = keys[(keys >> np.uint32(16)) == s] & np.uint32(0xffff)
    return int(np.bincount(low >> np.uint32(bits - min(BIN_BITS, bits))).max())


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    DeviceUtils.deallocate(d)


def sort_once(d, host):
    """One sort through the C ABI; returns (result, launch names, safety nets run, the low bits the finish sorted)."""
    lib = _lib.load()
    n = host.size
    tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    check(lib.adlhip_radix_sort_scratch_bytes_for(d._h, 0, n, 32, 1, ctypes.byref(tb), ctypes.byref(wb)), "scratch")
    bufs = [Buffer(d, n, np.uint32), Buffer(d, max(n, tb.value // 4), np.uint32), Buffer(d, wb.value, np.uint8)]
    try:
        bufs[0].write(host)
        runs0 = d.getParam("stat.net_runs")
        d.toggleProfiling(True)
        d.profile(reset=True)
        try:
            check(lib.adlhip_radix_sort_u32(d._h, bufs[0].ptr(), bufs[1].ptr(), bufs[2].ptr(), wb.value, n, 32), "sort")
            out = bufs[0].toHost()
        finally:
            prof = d.profile(reset=True)
            d.toggleProfiling(False)
        low_bits = int(bufs[2].toHost(4 * (DYN_LOW_BITS + 1)).view(np.uint32)[DYN_LOW_BITS])
        return out, set(prof), d.getParam("stat.net_runs") - runs0, low_bits
    finally:
        for b in bufs:
            b.release()


def run_case(d, name, keys, low_bits=16, tier=None):
    n = keys.size
    assert layout(n)[2] == tier, (name, layout(n))
    want = oracle.sort_u32(keys)
    got, names, nets, lb = sort_once(d, keys)
    assert names == LAUNCHES, (name, sorted(names))
    assert nets == 0, (name, "the safety net ran: the case did not reach the finish")
    assert lb == low_bits, (name, "low bits", lb)
    assert np.array_equal(got, want), name
    d.checkFault()
    assert d.getParam("debug.idle_dirty") == 0, name


def _place(targets, i, j, m):
    """a free segment for case (i, j): different pass-1 buckets and different places inside them"""
    s = ((37 * i + 83 * j + 5) % 256) * 256 + (7 * i + 101 * j + 3) % 256
    while s in targets:
        s = (s + 1) % SLOTS
    targets[s] = m
    return s


def _heavy_bin(seg, rng, bin_, h, distinct):
    """h keys of `seg` (all of it if it is smaller) in bin `bin_` of the 16-bit low half, none of the others in that bin"""
    other = (seg >> np.uint32(16 - BIN_BITS)) == bin_
    seg[other] ^= np.uint32(0x4000)   # another bin, 128 bins away
    h = min(h, seg.size)
    if distinct:
        r = np.sort(rng.permutation(BIN_SPAN)[:h])[::-1]   # descending: the transposition's worst case if placed in this order
    else:
        r = np.full(h, 0x55)
    at = rng.permutation(seg.size)[:h]
    seg[at] = (np.uint32(bin_ * BIN_SPAN) | r.astype(np.uint32))


SEAM_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 447, 448]


def test_the_cases_are_what_they_claim():
    """(CPU) the heavy bin holds exactly what was asked for and no other bin comes near the limit"""
    rng = np.random.default_rng(3)
    for bin_ in (0, (1 << BIN_BITS) - 1, 0xb3):
        for h in (MAX_ROUNDS - 1, MAX_ROUNDS, MAX_ROUNDS + 1):
            for distinct in (True, False):
                seg = rng.integers(0, 1 << 16, 448, dtype=np.uint32)
                _heavy_bin(seg, rng, bin_, h, distinct)
                c = np.bincount(seg >> np.uint32(16 - BIN_BITS), minlength=1 << BIN_BITS)
                assert c[bin_] == h and np.delete(c, bin_).max() < MAX_ROUNDS - 1
                assert np.unique(seg[(seg >> np.uint32(16 - BIN_BITS)) == bin_]).size == (h if distinct else 1)
    assert ((1 << BIN_BITS) - 1) * BIN_SPAN == 0xff80
    for m, rr in ((1535, 12), (1536, 12), (1025, 9)):
        starts = np.concatenate(([0], np.cumsum(_bin_sizes(m))))
        assert starts[-1] == m and not set(range(2 * rr, m, 2 * rr)) & set(starts.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("distinct", [True, False], ids=["distinct", "equal"])
def test_bin_size_edges_at_16Mi(dev, distinct):
    """<10,4>: in segments of every size around the seams of the blocked layout, one bin holds kFinish16MaxRounds - 1 keys (the
    last fast case), exactly kFinish16MaxRounds (the limit) and one more (the first that takes the LSD passes); the bin is the
    lowest, the highest (0xff80 ... 0xffff, beside the pads) or one in the middle; its keys are all distinct (descending) or all
    equal.  A segment smaller than the bin is the bin."""
    n = 16 * MI
    targets, cases = {}, {}
    i = 0
    for m in SEAM_SIZES:
        for bin_ in (0, (1 << BIN_BITS) - 1, 0xb3):
            for h in (MAX_ROUNDS - 1, MAX_ROUNDS, MAX_ROUNDS + 1):
                cases[_place(targets, i, h, m)] = (bin_, h)
                i += 1

    def patch(low, starts, rng):
        for s, (bin_, h) in cases.items():
            _heavy_bin(low[starts[s]:starts[s + 1]], rng, bin_, h, distinct)

    keys = build(counts_with(n, targets), 21 + distinct, patch)
    assert_fits(keys, n)
    s_limit = next(s for s, (b, h) in cases.items() if h == MAX_ROUNDS and targets[s] == 448)
    s_over = next(s for s, (b, h) in cases.items() if h == MAX_ROUNDS + 1 and targets[s] == 448)
    assert largest_bin(keys, s_limit) == MAX_ROUNDS and largest_bin(keys, s_over) == MAX_ROUNDS + 1
    run_case(dev, "bin edges 16Mi", keys, tier=1280)


@pytest.mark.gpu
def test_pad_collisions_at_16Mi(dev):
    """<10,4>: segments made wholly or mostly of 0xffff (the pad's value), of 0x0000, and of both -- and segments with as many of
    them as a bin may hold on the fast path, among random keys -- at 1, 129, 320 and 448 keys."""
    n = 16 * MI
    kinds = ("all_ffff", "all_0000", "mostly_ffff", "mostly_0000", "both", "both_and_some", "limit_ffff", "limit_0000", "limit_both")
    targets, cases = {}, {}
    for i, kind in enumerate(kinds):
        for j, m in enumerate((1, 129, 320, 448)):
            cases[_place(targets, i, j, m)] = kind

    def patch(low, starts, rng):
        for s, kind in cases.items():
            seg = low[starts[s]:starts[s + 1]]
            at = rng.permutation(seg.size)
            if kind.startswith("limit"):
                seg[seg >= np.uint32(0xff80)] -= np.uint32(0x1000)
                seg[seg < np.uint32(0x0080)] += np.uint32(0x1000)
                if kind != "limit_0000":
                    seg[at[:MAX_ROUNDS]] = 0xffff
                if kind != "limit_ffff":
                    seg[at[MAX_ROUNDS:2 * MAX_ROUNDS]] = 0x0000
                continue
            keep = 0 if kind.startswith("all") or kind == "both" else min(3, seg.size - 1)
            body = at[keep:]
            if kind.endswith("ffff"):
                seg[body] = 0xffff
            elif kind.endswith("0000"):
                seg[body] = 0x0000
            else:
                seg[body[: body.size // 2]] = 0xffff
                seg[body[body.size // 2:]] = 0x0000

    keys = build(counts_with(n, targets), 23, patch)
    assert_fits(keys, n)
    run_case(dev, "pads 16Mi", keys, tier=1280)


def _bin_sizes(m):
    """m keys over the 512 bins, 2 or 3 to a bin, the odd one out in bin 0 so that no bin starts where a lane's block starts (a
    full tile of 1536 keys would be 3 to every bin, which lines up with blocks of 24: there bin 0 holds 2 and the last bin 4)"""
    nb = 1 << BIN_BITS
    if m < 2 * nb:
        return np.array([1] * m + [0] * (nb - m))
    base = m // nb
    sizes = np.full(nb, base)
    sizes[1:1 + m % nb] += 1
    if m % nb == 0:
        sizes[0] -= 1
        sizes[-1] += 1
    elif m % nb == 1:
        sizes[0], sizes[1] = sizes[1], sizes[0]
    return sizes


@pytest.mark.gpu
def test_lane_boundaries_at_64Mi(dev):
    """<12,4>: segments of 1535, 1536, 1025 and 1 keys whose bins hold 2 - 3 keys each and straddle every boundary between two
    lanes' blocks (every even round exchanges across every boundary); the low halves are bin * 128 + r with r descending in
    key-value order across the segment."""
    n = 64 * MI
    targets, cases = {}, []
    for i, m in enumerate((1535, 1536, 1025, 1)):
        for c in range(3):
            cases.append(_place(targets, i, c, m))

    def patch(low, starts, rng):
        for s in cases:
            seg = low[starts[s]:starts[s + 1]]
            bins = np.repeat(np.arange(1 << BIN_BITS), _bin_sizes(seg.size))
            r = (seg.size - 1 - np.arange(seg.size)) % BIN_SPAN
            seg[:] = (bins * BIN_SPAN + r).astype(np.uint32)[rng.permutation(seg.size)]

    keys = build(counts_with(n, targets), 24, patch)
    assert_fits(keys, n)
    assert largest_bin(keys, cases[0]) == 3 and largest_bin(keys, cases[3]) == 4
    run_case(dev, "lane boundaries 64Mi", keys, tier=1536)


@pytest.mark.gpu
def test_the_2560_tile_at_72Mi(dev):
    """<20,4>: segments of 1792 (the slab's cap, 14 row pairs) and 1537 keys (13) with a bin of exactly kFinish16MaxRounds distinct
    keys, lowest, highest and in the middle."""
    n = 72 * MI
    targets, cases = {}, {}
    for i, m in enumerate((1792, 1537)):
        for j, bin_ in enumerate((0, (1 << BIN_BITS) - 1, 0xb3)):
            cases[_place(targets, i, j, m)] = bin_

    def patch(low, starts, rng):
        for s, bin_ in cases.items():
            _heavy_bin(low[starts[s]:starts[s + 1]], rng, bin_, MAX_ROUNDS, True)

    keys = build(counts_with(n, targets), 25, patch)
    assert_fits(keys, n)
    assert all(largest_bin(keys, s) == MAX_ROUNDS for s in cases)
    run_case(dev, "tile 2560", keys, tier=2560)


@pytest.mark.gpu
@pytest.mark.parametrize("b", [9, 10, 13])
def test_low_bits_9_to_15_at_16Mi(dev, b):
    """Keys confined to 2^(16 + b) values: the finish sorts b bits -- 9: the bin is the whole key (no rounds), 10: one bit below
    the bins, 13: four."""
    n = 16 * MI
    rng = np.random.default_rng(100 + b)
    keys = rng.integers(0, 1 << (16 + b), n, dtype=np.uint32)
    run_case(dev, "low bits %d" % b, keys, low_bits=b, tier=1280)
