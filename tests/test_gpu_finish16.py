"""The 16-bit LDS finish of the large u32 sort (finish16_kernels.hpp) (run with `-m gpu` on the MI355X box).

The finish sorts one segment per wave with a code path per number of row pairs (128 keys each), a validity test on the last row
pair only, and local passes that are skipped when a digit is constant.  Random keys at one size visit two or three of those
paths.  Here the keys are built segment by segment -- (segment << 16) | low -- so that chosen segments hold chosen counts and
chosen low halves.  The kernel has one form; the knob that once chose between two is gone, and setting it is an error.

Every case: bit-exact against the oracle's sort of the same keys; exactly the five launches of the cursor form with the wave
finish; the safety net has not run (a case that falls into it would test nothing); a clean fault word and an idle handle.
"""
import ctypes

import numpy as np
import pytest

import oracle
from oclradixsort_amd import Buffer, DeviceUtils, _lib
from oclradixsort_amd._lib import AdlHipError, check

MI = 1 << 20
SLOTS = 65536
LAUNCHES = {"msd2_sample", "msd2_pass1_u32", "msd2_pass2_u32", "msd2_offsets", "segment_sort_wave_u32"}
DYN_LOW_BITS = 4   # hybrid_kernels.hpp kDynLowBits: word of the work buffer's first block that holds the bits the finish sorts


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
    """(segment << 16) | random low half, counts[s] keys in segment s; patch(low, starts) may rewrite the low halves of chosen
    segments in place; then a stride permutation spreads every segment over the whole input."""
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


def fits(keys, n):
    """The CPU check before anything is sent: no bucket beyond its pass-1 slab, no segment beyond its slab."""
    stride_a, stride_b, _ = layout(n)
    seg = np.bincount(keys >> np.uint32(16), minlength=SLOTS)
    return int(seg.max()) <= stride_b and int(seg.reshape(256, 256).sum(axis=1).max()) <= stride_a


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


def run_case(d, name, keys, want=None, low_bits=16, tier=None, times=1):
    n = keys.size
    if tier is not None:
        assert layout(n)[2] == tier, (name, layout(n))
    want = oracle.sort_u32(keys) if want is None else want
    for t in range(times):
        got, names, nets, lb = sort_once(d, keys)
        tag = (name, "run", t)
        assert names == LAUNCHES, (tag, sorted(names))
        assert nets == 0, (tag, "the safety net ran: the case did not reach the finish")
        assert lb == low_bits, (tag, "low bits", lb)
        assert np.array_equal(got, want), tag
        d.checkFault()
        assert d.getParam("debug.idle_dirty") == 0, tag


def test_the_builder_keeps_its_counts():
    """(CPU) the counts of the built keys are the counts asked for, and the slab check sees an overfull segment"""
    n = 1 << 20
    c = counts_with(n, {5: 0, 6: 1, 7: 40, 65535: 3})
    keys = build(c, 1)
    assert np.array_equal(np.bincount(keys >> np.uint32(16), minlength=SLOTS), c)
    assert layout(16 * MI) == (102400, 448, 1280) and layout(64 * MI) == (397312, 1536, 1536) and layout(72 * MI) == (446464, 1792, 2560)
    assert fits(build(counts_with(16 * MI, {9: 448}), 2), 16 * MI)
    assert not fits(build(counts_with(16 * MI, {9: 449}), 2), 16 * MI)


def _spread(values, copies=3):
    """{segment: count}: every value in `copies` segments, in different pass-1 buckets and at different places inside them"""
    t = {}
    for i, v in enumerate(values):
        for c in range(copies):
            s = ((37 * i + 83 * c + 5) % 256) * 256 + (i * 7 + c * 101 + 3) % 256
            while s in t:
                s = (s + 1) % SLOTS
            t[s] = v
    return t


@pytest.mark.gpu
def test_every_row_count_at_64Mi(dev):
    """<12,4>: slab = tile = 1536.  Segments of 128 r - 1, 128 r and 128 r + 1 keys for every row-pair count r = 1 ... 12 (the
    tile's cap 1536 is r = 12; one key more would not fit the slab), and of 0, 1 and 2 keys."""
    n = 64 * MI
    sizes = [0, 1, 2] + [m for r in range(1, 13) for m in (128 * r - 1, 128 * r, 128 * r + 1) if m <= 1536]
    assert 1536 in sizes and 1535 in sizes and len(sizes) == 38
    keys = build(counts_with(n, _spread(sizes)), 11)
    assert fits(keys, n)
    run_case(dev, "rows 64Mi", keys, tier=1536)


@pytest.mark.gpu
def test_last_row_pair_and_constant_bytes_at_16Mi(dev):
    """<10,4>: slab 448 in the 1280 tile.  Last row pair with one lane, only its low half, its low half and one lane more, or
    all of it valid (both layouts: as loaded, two keys to a dword, and as placed, 64 keys to a row); segments whose low 16 bits
    are all equal (no local pass runs: the unplaced stores), whose low or high byte is constant (one pass skipped, each way
    round), and the same with a single key that differs."""
    n = 16 * MI
    sizes = [1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 168, 191, 192, 193, 194, 255, 256, 257, 258, 300, 319, 320, 321, 383,
             384, 385, 386, 447, 448]
    targets = _spread(sizes)
    kinds = ("equal", "low_const", "high_const", "equal_but_one_low", "equal_but_one_high", "equal_but_one_both",
             "low_const_but_one", "high_const_but_one")
    const = {}
    for i, kind in enumerate(kinds):
        for j, m in enumerate((1, 2, 129, 192, 256, 321, 448)):
            s = ((11 * i + 29 * j + 100) % 256) * 256 + (13 * i + 31 * j + 40) % 256
            while s in targets:
                s += 1
            targets[s] = m
            const[s] = kind

    def patch(low, starts, rng):
        for s, kind in const.items():
            seg = low[starts[s]:starts[s + 1]]
            one = int(rng.integers(0, seg.size))
            if kind.startswith("equal"):
                seg[:] = 0x3c5a
                if kind.endswith("one_low"):
                    seg[one] = 0x3c5b
                elif kind.endswith("one_high"):
                    seg[one] = 0x3d5a
                elif kind.endswith("one_both"):
                    seg[one] = 0xc3a5
            elif kind.startswith("low_const"):
                seg[:] = (seg & np.uint32(0xff00)) | np.uint32(0x77)
                if kind.endswith("but_one"):
                    seg[one] ^= np.uint32(0x01)
            else:
                seg[:] = (seg & np.uint32(0x00ff)) | np.uint32(0x5500)
                if kind.endswith("but_one"):
                    seg[one] ^= np.uint32(0x8000)

    keys = build(counts_with(n, targets), 12, patch)
    assert fits(keys, n)
    run_case(dev, "edges 16Mi", keys, tier=1280)


@pytest.mark.gpu
def test_constant_bytes_at_64Mi(dev):
    """The same where a segment has 8 row pairs and more: the segments of the lower half of the key range have a constant low
    byte, those of the upper half a constant high byte (every segment skips one pass), full tiles among them."""
    n = 64 * MI
    counts = counts_with(n, _spread([1536, 1535, 1025, 1024, 1023, 1]))

    def patch(low, starts, rng):
        h = starts[SLOTS // 2]
        low[:h] = (low[:h] & np.uint32(0xff00)) | np.uint32(0xa5)
        low[h:] = (low[h:] & np.uint32(0x00ff)) | np.uint32(0x0100)

    keys = build(counts, 13, patch)
    assert fits(keys, n)
    run_case(dev, "constant bytes 64Mi", keys, tier=1536)


@pytest.mark.gpu
@pytest.mark.parametrize("bits,prefix", [(28, 0x5), (27, 0), (24, 0)])
def test_low_bits_below_16_at_16Mi(dev, bits, prefix):
    """Keys confined to 2^bits values (under a common prefix): the sample places the two digits lower and the finish sorts
    bits - 16 bits -- 12 in two passes of 6, 11 in passes of 6 and 5, 8 in one pass."""
    n = 16 * MI
    rng = np.random.default_rng(bits)
    keys = rng.integers(0, 1 << bits, n, dtype=np.uint32) | np.uint32(prefix << bits)
    run_case(dev, "low bits %d" % (bits - 16), keys, low_bits=bits - 16, tier=1280)


@pytest.mark.gpu
def test_the_2560_tile_at_72Mi(dev):
    """<20,4>: 72 Mi keys sit in the 2560 tile with slabs of 1792 keys; segments of 13 and 14 row pairs (the slab's cap) beside
    the typical 9 and 10."""
    n = 72 * MI
    sizes = [0, 1, 1536, 1537, 1663, 1664, 1665, 1791, 1792]
    keys = build(counts_with(n, _spread(sizes)), 14)
    assert fits(keys, n)
    run_case(dev, "tile 2560", keys, tier=2560)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mi", [16, 64])
def test_uniform_keys_twice_on_one_handle(dev, n_mi):
    with pytest.raises(AdlHipError, match="unknown parameter"):   # the retired A/B knob; the handle sorts on as before
        dev.setParam("debug.finish16_alg", 1)
    n = n_mi * MI
    keys = oracle.keys_u32(n, seed=n_mi)
    run_case(dev, "uniform %d Mi" % n_mi, keys, tier=1280 if n_mi == 16 else 1536, times=2)
