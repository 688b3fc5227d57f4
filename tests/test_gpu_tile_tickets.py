"""The persistent passes of the large keys-only sort (cursor form, "sort.msd2" = 4) hand out their tiles by ticket: a workgroup's
first two tiles are static, every later one is drawn from a counter in the handle -- one counter for pass 1, one per XCD for pass 2,
where an XCD's full tiles come first and its remainder tiles last, largest first.  At the default grid a sort of fewer than six rounds
of tiles runs the static kernels of before; with "debug.persist_grid" set the grid is small, small inputs give every workgroup
many rounds, and the tickets are drawn at every size (from a workgroup's third tile on).  Every result is compared bit-exactly
with the oracle; where the input fits the slabs the safety net must not have run (it would hide a wrong queue), and where it
cannot fit it must have.  "debug.idle_dirty" says nothing about the ticket counters (they lie behind the region the idle table
covers and are reset on entry): that they are reset is shown by the results of the sequences alone.
"""
import numpy as np
import pytest

import oracle
from oclradixsort_amd import AdlHipError, Buffer, DeviceUtils, Pprims

pytestmark = pytest.mark.gpu

TILE32 = 16384   # keys per tile of the persistent passes: u32 keys
TILE64 = 8192    # u64 keys


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    DeviceUtils.deallocate(d)


@pytest.fixture()
def pp(dev):
    before = {k: dev.getParam(k) for k in ("sort.msd2", "sort.mid", "debug.persist_grid")}
    # the passes are launched under the same names as persistent kernels and as one tile per workgroup: the persistent ones run
    # while "sort.persist" is 1 and the slabs stay below 4 GiB, which every size here does by a factor of ten
    assert dev.getParam("sort.persist") == 1
    dev.setParam("sort.msd2", 4)
    dev.setParam("sort.mid", 0)   # (the mid-size sort would take u32 keys up to its limit)
    p = Pprims()
    yield p
    p.close()
    for k, v in before.items():
        dev.setParam(k, v)


def _sort(dev, p, keys):
    wide = keys.dtype == np.uint64
    b = Buffer(dev, keys.size, keys.dtype)
    try:
        b.write(keys)
        (p.radixSort64 if wide else p.radixSort)(dev, b, keys.size)
        return b.toHost()
    finally:
        b.release()


def _check(dev, p, keys, net):
    """Sort, compare with the oracle; the persistent passes must have been launched; net: whether the safety net must (True) or
    must not (False) have run."""
    before = dev.getParam("stat.net_runs")
    dev.toggleProfiling(True)
    dev.profile(reset=True)
    try:
        got = _sort(dev, p, keys)
    finally:
        prof = dev.profile(reset=True)
        dev.toggleProfiling(False)
    kind = "u64" if keys.dtype == np.uint64 else "u32"
    assert {"msd2_sample", "msd2_pass1_" + kind, "msd2_pass2_" + kind, "msd2_offsets"} <= set(prof), prof
    want = oracle.sort_u64(keys) if keys.dtype == np.uint64 else oracle.sort_u32(keys)
    assert np.array_equal(got, want)
    assert (dev.getParam("stat.net_runs") != before) == net
    assert dev.getParam("debug.idle_dirty") == 0, "word %#x" % dev.getParam("debug.idle_first")


def _round_sizes(grid):
    return [5 * TILE32 + 3,                    # fewer tiles than workgroups (grid 8 and 16)
            grid * TILE32,                     # exactly one round
            grid * TILE32 + 1,                 # one key into the second round
            2 * grid * TILE32 - 1,             # the last tile of the second round one key short
            5 * grid * TILE32 + TILE32 // 2,   # five rounds (two static, three drawn), half a tile at the end
            7 * grid * TILE32 + 5,
            3 * grid * TILE32 + 4099]          # not a multiple of 4: the last 16-byte load is cut


@pytest.mark.parametrize("grid", [8, 16])
def test_sizes_around_the_rounds(dev, pp, grid):
    dev.setParam("debug.persist_grid", grid)
    for i, n in enumerate(_round_sizes(grid)):
        _check(dev, pp, oracle.keys_u32(n, seed=40 + i), net=False)


def _queue_keys():
    """u32 keys whose top byte is chosen: bucket b (served by XCD b % 8 in pass 2) gets sizes[b] keys with random low bits."""
    T = TILE32
    # most buckets: two tiles, the second short by a different amount each (remainders of many sizes, a few of them equal)
    sizes = np.array([2 * T - (b * 37) % 3000 for b in range(256)], dtype=np.int64)
    sizes[0], sizes[8], sizes[16] = T, 2 * T, 2 * T          # exactly k tiles: no remainder tile
    sizes[24], sizes[32] = T + 1, 2 * T + 1                  # a remainder of one key
    sizes[40], sizes[48] = T - 1, 2 * T - 1                  # one key short
    sizes[56], sizes[64], sizes[72] = 1, 100, T // 2         # less than a tile
    sizes[80] = sizes[88] = sizes[1] = sizes[250] = 0        # empty buckets
    sizes[3::8] = 0                                          # XCD 3: nothing at all
    sizes[5::8] = 0                                          # XCD 5: one bucket
    sizes[133] = 2 * T + 17
    # 63 of the 256 buckets are empty, so the slabs (1.5 x the MEAN bucket and segment) leave the two-tile buckets a few per cent
    # only: the second byte goes round within a bucket, which fills its segments evenly; the low 16 bits are random
    rng = np.random.default_rng(20250101)
    top = np.repeat(np.arange(256, dtype=np.uint32), sizes)
    within = np.arange(top.size, dtype=np.int64) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    keys = (top << np.uint32(24)) | ((within & 255).astype(np.uint32) << np.uint32(16)) | rng.integers(0, 1 << 16, size=top.size, dtype=np.uint32)
    rng.shuffle(keys)
    return keys


@pytest.fixture(scope="module")
def queue_keys():
    keys = _queue_keys()
    keys.setflags(write=False)
    return keys


@pytest.mark.parametrize("grid", [8, 16])
def test_pass2_queues(dev, pp, queue_keys, grid):
    """Full tiles only, remainders of 1 ... TILE - 1 keys, buckets below a tile, empty buckets, an XCD without keys and one with a
    single bucket, in one input that fits its slabs (about 6 Mi keys)."""
    dev.setParam("debug.persist_grid", grid)
    _check(dev, pp, queue_keys, net=False)


@pytest.mark.parametrize("grid", [8, 16])
def test_net_path(dev, pp, grid):
    """Keys that cannot fit the slabs: all equal (the sample kernel's repeat screen: the passes leave before they draw a ticket) and
    one heavy top byte (a slab overflows while the passes run: the workgroups leave between two tiles)."""
    dev.setParam("debug.persist_grid", grid)
    n = 7 * grid * TILE32 + TILE32 // 2
    _check(dev, pp, np.full(n, 0x9e3779b9, dtype=np.uint32), net=True)
    keys = oracle.keys_u32(n, seed=77)
    keys[::2] = (keys[::2] & np.uint32(0x00ffffff)) | np.uint32(0x42000000)
    _check(dev, pp, keys, net=True)


def test_sequence_on_one_handle(dev, pp):
    """The counters are reset on entry, whatever the sort before left in them: uniform, all equal, uniform, uniform with another grid."""
    n = 7 * 8 * TILE32 + TILE32 // 2
    dev.setParam("debug.persist_grid", 8)
    _check(dev, pp, oracle.keys_u32(n, seed=50), net=False)
    _check(dev, pp, np.full(n, 12345, dtype=np.uint32), net=True)
    _check(dev, pp, oracle.keys_u32(n, seed=51), net=False)
    dev.setParam("debug.persist_grid", 16)
    _check(dev, pp, oracle.keys_u32(n, seed=52), net=False)


@pytest.mark.parametrize("tiles", [40, 7 * 8 + 1])
def test_u64_keys(dev, pp, tiles):
    """Five rounds and seven, the last one key long: both draw (the grid is set)."""
    dev.setParam("debug.persist_grid", 8)
    _check(dev, pp, oracle.keys_u64(tiles * TILE64 - (TILE64 - 1 if tiles != 40 else 0), seed=60), net=False)


def test_default_grid_crosses_a_round(dev, pp):
    """Three rounds at the shipped grid: the STATIC kernels (fewer than six rounds), crossing a round boundary.  Nothing is drawn."""
    dev.setParam("debug.persist_grid", 0)
    n = 3 * (2 * int(dev.info.compute_units)) * TILE32 + 12345
    _check(dev, pp, oracle.keys_u32(n, seed=61), net=False)


def test_default_grid_draws(dev, pp):
    """Six rounds at the shipped grid, the smallest sort that draws there (about 50 Mi keys): the drawing kernels as they ship."""
    dev.setParam("debug.persist_grid", 0)
    n = 6 * (2 * int(dev.info.compute_units)) * TILE32 + 12345
    _check(dev, pp, oracle.keys_u32(n, seed=62), net=False)


def test_knob(dev):
    assert dev.getParam("debug.persist_grid") == 0
    try:
        dev.setParam("debug.persist_grid", 16)
        assert dev.getParam("debug.persist_grid") == 16
        with pytest.raises(AdlHipError):
            dev.setParam("debug.persist_grid", -1)
        with pytest.raises(AdlHipError):
            dev.setParam("debug.persist_grid", 4097)
        dev.setParam("debug.persist_grid", 4096)
        assert dev.getParam("debug.persist_grid") == 4096
        dev.setParam("debug.persist_grid", 16)
        assert dev.getParam("debug.persist_grid") == 16
    finally:
        dev.setParam("debug.persist_grid", 0)
    assert dev.getParam("debug.persist_grid") == 0
