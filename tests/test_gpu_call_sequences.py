"""Every sort path leaves the handle's device state idle, whatever ran before it and whatever runs next.

The fast paths keep device words that belong to the HANDLE (adlhip.hip kIdleTable: cursors, flags, counters and sample words of
the large sort, the mid-size sort's histograms and cursors, the dictionary block, the fault words).  A word left dirty rarely
spoils the sort that dirtied it; it changes what the NEXT sort on that handle does.  So this file queues calls of different kinds
back to back on one long-lived handle -- one shared d_tmp, one shared d_work, no synchronisation in between, as bench.py and any
real caller drive the library -- and after every batch checks three things: every result is bit-exact against a host reference,
the safety net ran exactly as often as the same calls cause on a fresh handle ("stat.net_runs" / "stat.net_counting"), and
"debug.idle_dirty" finds every idle-valued word at its value.

A state is one row of STATES: a call, its element kind, n, sort_bits, knobs, work size, key recipe, the kernel labels it must
launch and what its safety net must do.  Calibration runs each state alone on a fresh handle and asserts those claims; the matrix
runs every ordered pair; seeded walks run longer chains; the last tests repeat the large-sort states on the handle the matrix
used, and queue sorts behind a call that raises the software fault word.  Everything goes through the C ABI.
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

Mi = 1 << 20
U32, KV32, U64, SOA32 = 0, 1, 2, 3
ESZ = {U32: 4, KV32: 8, U64: 8, SOA32: 4}
MAX_BITS = {U32: 32, KV32: 32, U64: 64, SOA32: 32}
REGION_NAME = {1: "d_msd2", 2: "d_mid_hist", 3: "d_dict", 4: "d_fault"}
MSD2_FLAG = 8192 + 65536          # d_msd2: flag = base + MSD2_FLAG (adlhip.hip kMsd2Flag)
MID_STATE = 16 * 1024             # d_mid_hist: the two-launch form's state (adlhip.hip kMidState)

DEFAULT_KNOBS = {"sort.algo": -1, "sort.digit_bits": 8, "sort.tile": -1, "sort.msd2": 1, "sort.mid": 1, "sort.dict": 1,
                 "sort.binfinish": 1, "sort.net_lookback": 1, "partition.lookback": 1}

N_LARGE = 3 * Mi + 17             # the large sort's states
N_MID = 300007                    # the mid-size forms
NET_NONE, NET_LSD, NET_COUNTING = "none", "lsd", "counting"


def align_up(x, a):
    return (x + a - 1) // a * a


def _lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


# ---------------------------------------------------------------------------------------------
# key recipes (tests/test_gpu_memory_contract.py make_keys, tests/test_gpu_parity.py)
# ---------------------------------------------------------------------------------------------
def _uniform(width, n, seed):
    return oracle.keys_u32(n, seed=seed) if width == 32 else oracle.keys_u64(n, seed=seed)


def make_keys(width, n, recipe, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint32 if width == 32 else np.uint64
    top = np.uint64(0xFFFFFFFFFFFFFFFF) if width == 64 else np.uint32(0xFFFFFFFF)
    u = _uniform(width, n, seed)
    if recipe == "uniform":
        return u
    if recipe in ("few256", "dict4096", "few16"):
        d = {"few256": 256, "dict4096": 4096, "few16": 16}[recipe]
        vals = rng.integers(1, int(top), d, dtype=dt, endpoint=False)
        vals[0], vals[1] = 0, top           # 0 and the all-ones key among them
        return vals[rng.integers(0, d, n)]
    if recipe == "five":                    # five values: the sample flags repeats before the passes move a key
        return ((u % dt(5)) * dt(0x01010101)).astype(dt)
    if recipe == "few_plus_unseen":         # 40 values and one key no sample sees: the dictionary misses, LSD passes sort
        vals = rng.integers(1, int(top), 40, dtype=dt, endpoint=False)
        k = vals[rng.integers(0, 40, n)]
        k[(n * 5) // 12 + 3] = dt(0x01234567)
        return k
    if recipe == "heavy":                   # one top byte holds ~90 % of the keys, the bits below vary
        sel = rng.random(n) < 0.9
        k = u.copy()
        if width == 32:
            k[sel] = (k[sel] & np.uint32(0x00FFFFFF)) | np.uint32(0x5A000000)
        else:
            k[sel] = (k[sel] & np.uint64(0x00FFFFFFFFFFFFFF)) | np.uint64(0x5A << 56)
        return k
    if recipe == "heavy_low":               # nine keys in ten below 2^24 (mid-size sort: a bucket beyond the LDS tile)
        return np.where(np.arange(n) % 10 != 0, u >> dt(8), u).astype(dt)
    if recipe == "below24":                 # the top byte is constant
        return (u >> dt(8)).astype(dt)
    if recipe == "eighth":                  # one eighth of the key range: the digits are placed from the sample
        return ((u >> dt(3)) | dt(0xA0000000)).astype(dt)
    if recipe == "outliers":                # keys below 2^24 and two above what the sample shows: a pass overflows
        k = (u >> dt(8)).copy()
        k[12345] = dt(0xF0000001)
        k[n - 2] = dt(0x80000000)
        return k
    if recipe == "dups64":                  # u64 keys that vary in their top 16 and low 8 bits only: segments full of duplicates
        return (u & np.uint64(0xFFFF0000000000FF)).astype(np.uint64)
    raise ValueError(recipe)


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
# the states
# ---------------------------------------------------------------------------------------------
class State:
    def __init__(self, name, call, kind, n, bits, knobs, level, recipe, labels, net, large=False, refused=None, extra=None):
        self.name, self.call, self.kind, self.n, self.bits, self.knobs = name, call, kind, n, bits, knobs
        self.level, self.recipe, self.labels, self.net, self.large, self.refused = level, recipe, set(labels), net, large, refused
        self.extra = extra or {}
        self.seed = 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 9000
        self._built = None

    # -- host side: arrays of the call (name, initial contents), expected contents afterwards ---------------------------------
    def build(self):
        """[(array name, initial bytes, expected bytes)] in the order the image lays them out; cached."""
        if self._built is None:
            self._built = [(nm, np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1))
                           for nm, a, w in self._arrays()]
        return self._built

    def _arrays(self):
        n, bits, kind = self.n, self.bits, self.kind
        idx = np.arange(n, dtype=np.uint64)
        if self.call == "sort":
            keys = make_keys(64 if kind == U64 else 32, n, self.recipe, self.seed)
            if self.refused:
                return [("data", keys, keys)]
            if kind == KV32:
                arr = keys.astype(np.uint64) | (idx << np.uint64(32))
                want = arr[stable_order(keys, bits)]       # = the oracle's stable sort (tests/test_oracle.py) on whole keys
            elif bits == MAX_BITS[kind]:
                arr, want = keys, (oracle.sort_u32(keys) if kind == U32 else np.sort(keys))
            else:
                arr, want = keys, keys[stable_order(keys, bits)]
            return [("data", arr, want)]
        if self.call == "soa32":
            keys = make_keys(32, n, self.recipe, self.seed)
            vals = idx.astype(np.uint32)
            order = stable_order(keys, bits)
            return [("keys", keys, keys[order]), ("vals", vals, vals[order])]
        if self.call == "soa":               # u64 keys, 16-byte values
            keys = make_keys(64, n, self.recipe, self.seed)
            lo = idx.astype(np.uint32)
            vals = np.stack([lo, ~lo, np.full(n, 0xB0BAFE77, np.uint32), (idx * np.uint64(3)).astype(np.uint32)], axis=1)
            order = stable_order(keys, bits)
            return [("keys", keys, keys[order]), ("vals", vals, vals[order])]
        if self.call == "scan":
            src = np.random.default_rng(self.seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            want, total = oracle.exclusive_scan_u32(src)
            self.extra["total"] = int(total)
            return [("src", src, src), ("dst", np.full(n, 0xA5A5A5A5, np.uint32), want)]
        if self.call in ("top_byte", "msb"):
            keys = make_keys(32, n, self.recipe, self.seed)
            arr = keys if kind == U32 else keys.astype(np.uint64) | (idx << np.uint64(32))
            buckets = 256 if self.call == "top_byte" else self.extra["buckets"]
            top = keys.astype(np.uint64) >> np.uint64(24)      # stable by the top byte, which refines the buckets without mixing them
            order = (np.sort((top << np.uint64(32)) | idx) & np.uint64(0xFFFFFFFF)).astype(np.int64)
            bucket = (keys.astype(np.uint64) >> np.uint64(32 - (buckets.bit_length() - 1))).astype(np.int64)
            counts = np.bincount(bucket, minlength=buckets).astype(np.uint32)
            return [("in", arr, arr), ("out", np.full(arr.size, 0xA5, arr.dtype), arr[order]),
                    ("counts", np.full(buckets, 0xA5A5A5A5, np.uint32), counts)]
        if self.call == "segsort":
            low_bits, bound = self.bits, 16384
            rng = np.random.default_rng(self.seed)
            sizes = np.concatenate([[0, bound, 1, 0, 0], rng.integers(0, bound + 1, 40), [bound - 1, 0, bound]]).astype(np.int64)
            lo = 1237                                  # the segments cover [lo, hi) of a larger array
            starts = (lo + np.concatenate([[0], np.cumsum(sizes)])).astype(np.uint32)
            hi = int(starts[-1])
            arr = oracle.keys_u32(hi + 3001, seed=self.seed)
            want = arr.copy()
            seg = arr[lo:hi]
            seg_id = np.repeat(np.arange(sizes.size, dtype=np.uint64), sizes)
            low = seg.astype(np.uint64) & np.uint64((1 << low_bits) - 1)
            want[lo:hi] = seg[np.argsort((seg_id << np.uint64(32)) | low, kind="stable")]
            self.extra.update(num_segments=starts.size - 1, bound=bound)
            return [("data", arr, want), ("seg_start", starts, starts)]
        raise ValueError(self.call)

    def offsets(self):
        offs, at = {}, 0
        for nm, a, _ in self.build():
            offs[nm] = at
            at = align_up(at + a.size, 256)
        return offs, at

    def image(self, which):
        """The state's arrays laid out at 256-byte offsets: which = 1 the initial contents, 2 the expected ones."""
        offs, total = self.offsets()
        img = np.zeros(total, np.uint8)
        for t in self.build():
            img[offs[t[0]]:offs[t[0]] + t[which].size] = t[which]
        return img


LARGE_CURSOR = {"msd2_sample", "msd2_pass1_u32", "msd2_pass2_u32", "msd2_offsets"}
LARGE_HYBRID = {"msd2s_prep", "msd2s_pass1_u32", "msd2h_pass2_u32", "msd2s_offsets"}
STABLE_U32 = {"msd2s_prep", "msd2s_pass1_u32", "msd2s_pass2_u32", "msd2s_offsets"}
STABLE_U64 = {"msd2s_prep", "msd2s_pass1_u64", "msd2s_pass2_u64", "msd2s_offsets"}
STABLE_KV = {"msd2s_prep", "msd2s_pass1_kv32", "msd2s_pass2_kv32", "msd2s_offsets", "segment_sort_wave_e64"}
THREE_KERNEL = {"count_u32_8b", "scan_table", "scatter_u32_8b"}
MID2 = {"mid_bucket_scatter_u32", "segment_sort_u32"}


def _S(*a, **k):
    return State(*a, **k)


STATES = [
    # name, call, kind, n, sort_bits, knobs, work level, key recipe, claimed labels, claimed net
    _S("small-u32", "sort", U32, 6001, 32, {}, 1, "uniform", {"small_sort_u32"}, NET_NONE),
    _S("small-pairs", "sort", KV32, 9001, 32, {}, 1, "uniform", {"small_sort_e64"}, NET_NONE),
    _S("mid2-friendly", "sort", U32, N_MID, 32, {"sort.mid": 2}, 1, "uniform", MID2, NET_NONE),
    _S("mid2-below-2^24", "sort", U32, N_MID, 32, {"sort.mid": 2}, 1, "below24", MID2, NET_NONE),
    _S("mid3-friendly-pairs", "sort", KV32, N_MID, 32, {"sort.mid": 3}, 1, "uniform", {"mid_prep_e64", "onesweep_e64_8b", "segment_sort_e64"}, NET_NONE),
    _S("mid3-skewed", "sort", U32, N_MID, 32, {"sort.mid": 3}, 1, "heavy_low", {"mid_prep_u32", "onesweep_u32_8b", "segment_sort_u32"}, NET_NONE),
    _S("three-kernel-20-bits", "sort", U32, Mi + 5, 20, {"sort.algo": 1}, 1, "uniform", THREE_KERNEL | {"scatter_u32_4b"}, NET_NONE),
    _S("one-sweep-u64", "sort", U64, Mi + 1, 64, {"sort.algo": 0}, 1, "uniform", {"os_hist_e64", "os_tables", "onesweep_e64_8b"}, NET_NONE),
    _S("level-0-work", "sort", U32, N_LARGE, 32, {}, 0, "uniform", THREE_KERNEL, NET_NONE),
    _S("level-2-work-lean", "sort", U32, 6 * Mi + 3, 32, {}, 2, "uniform", LARGE_CURSOR, NET_NONE, large=True),
    _S("cursor-friendly", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "uniform", LARGE_CURSOR, NET_NONE, large=True),
    _S("cursor-one-eighth", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "eighth", LARGE_CURSOR, NET_NONE, large=True),
    _S("cursor-outliers", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "outliers", LARGE_CURSOR, NET_LSD, large=True),
    _S("cursor-heavy-count-scan-scatter", "sort", U32, N_LARGE, 32, {"sort.msd2": 4, "sort.net_lookback": 0}, 1, "heavy", LARGE_CURSOR, NET_LSD,
       large=True),
    _S("cursor-five-values", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "five", LARGE_CURSOR, NET_COUNTING, large=True),
    _S("cursor-4096-values", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "dict4096", LARGE_CURSOR, NET_COUNTING, large=True),
    _S("cursor-dictionary-miss", "sort", U32, N_LARGE, 32, {"sort.msd2": 4}, 1, "few_plus_unseen", LARGE_CURSOR, NET_LSD, large=True),
    _S("hybrid-friendly", "sort", U32, N_LARGE, 32, {"sort.msd2": 5}, 1, "uniform", LARGE_HYBRID, NET_NONE, large=True),
    _S("hybrid-overflowing", "sort", U32, N_LARGE, 32, {"sort.msd2": 5}, 1, "outliers", LARGE_HYBRID, NET_LSD, large=True),
    _S("stable-u32-24-bits", "sort", U32, N_LARGE, 24, {"sort.msd2": 2}, 1, "uniform", STABLE_U32, NET_NONE, large=True),
    _S("stable-u64-44-bits", "sort", U64, N_LARGE, 44, {}, 1, "uniform", STABLE_U64, NET_NONE, large=True),
    _S("stable-u64-binfinish-2", "sort", U64, N_LARGE, 64, {"sort.msd2": 3, "sort.binfinish": 2}, 1, "dups64",
       STABLE_U64 | {"segment_sort_bin_u64", "segment_sort_listed_e64"}, NET_NONE, large=True),
    _S("stable-u64-binfinish-0", "sort", U64, N_LARGE, 64, {"sort.msd2": 3, "sort.binfinish": 0}, 1, "uniform",
       STABLE_U64 | {"segment_sort_wave_e64"}, NET_NONE, large=True),
    _S("pairs-friendly", "sort", KV32, N_LARGE, 32, {"sort.msd2": 2}, 1, "uniform", STABLE_KV, NET_NONE, large=True),
    _S("pairs-skewed", "sort", KV32, N_LARGE, 32, {"sort.msd2": 2}, 1, "heavy", STABLE_KV - {"segment_sort_wave_e64"}, NET_LSD, large=True),
    _S("pairs-16-valued-keys", "sort", KV32, N_LARGE, 32, {"sort.msd2": 2}, 1, "few16", STABLE_KV - {"segment_sort_wave_e64"}, NET_COUNTING,
       large=True),
    _S("pairs-rank-0", "sort", KV32, N_LARGE, 32, {"sort.msd2": 2, "sort.rank": 0}, 1, "uniform", STABLE_KV, NET_NONE, large=True),
    _S("soa32-large", "soa32", SOA32, N_LARGE, 32, {}, 1, "uniform", {"msd2s_prep", "msd2s_pass1_soa", "msd2s_pass2_soa", "msd2s_offsets"}, NET_NONE,
       large=True),
    _S("soa-u64-keys-16-byte-values", "soa", U64, Mi + Mi // 2 + 17, 64, {}, 1, "uniform", {"soa_pack_index_k64", "soa_repack_high", "soa_gather"},
       NET_NONE),
    _S("scan", "scan", U32, Mi + 5, 0, {}, 1, None, {"scan_reduce", "scan_partials", "scan_apply"}, NET_NONE),
    _S("partition-top-byte-8Mi", "top_byte", U32, 8 * Mi, 32, {}, 1, "uniform", {"os_hist_u32", "os_tables", "onesweep_u32_8b"}, NET_NONE),
    _S("partition-msb-pairs-small", "msb", KV32, 4097, 32, {}, 0, "uniform", {"count_e64_8b", "scan_table", "scatter_e64_8b", "fold_buckets"}, NET_NONE,
       extra={"buckets": 16}),
    _S("segment-sort", "segsort", U32, 0, 24, {}, None, None, {"segment_sort_u32"}, NET_NONE),
    _S("refused-unaligned-work", "sort", U32, N_LARGE, 32, {}, 1, "uniform", set(), NET_NONE, refused="work+4"),
    _S("refused-sort-bits-6", "sort", U32, N_LARGE, 6, {}, 1, "uniform", set(), NET_NONE, refused="bits"),
]
STATE_BY_NAME = {s.name: s for s in STATES}
assert len(STATE_BY_NAME) == len(STATES)
MID_STATES = ["mid2-friendly", "mid2-below-2^24", "mid3-friendly-pairs", "mid3-skewed"]


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
def set_knobs(dev, knobs):
    for k, v in DEFAULT_KNOBS.items():
        dev.setParam(k, knobs.get(k, v))
    dev.setParam("sort.rank", knobs.get("sort.rank", dev.getParam("sort.lds_ordered")))


def net_stats(dev):
    return dev.getParam("stat.net_runs"), dev.getParam("stat.net_counting")


def sync(dev):
    rc = _lib.load().adlhip_sync(dev._h)
    assert rc == 0, "adlhip_sync reported: %s" % _lib_err()


def dmalloc(dev, nbytes):
    p = ctypes.c_void_p()
    check(_lib.load().adlhip_malloc(dev._h, nbytes, ctypes.byref(p)), "adlhip_malloc")
    return p.value


def decode_idle(first):
    region, word = first >> 24, first & 0xFFFFFF
    where = "word %d" % word
    if region == 1 and word >= MSD2_FLAG:
        where = "flag[%d]" % (word - MSD2_FLAG)
    elif region == 1:
        where = "first-pass cursor word %d" % word if word < 8192 else "second-pass cursor %d" % (word - 8192)
    elif region == 2 and word >= MID_STATE:
        where = "two-launch state[%d]" % (word - MID_STATE)
    return "%s %s" % (REGION_NAME.get(region, "region %d" % region), where)


def assert_idle(dev, what):
    dirty = dev.getParam("debug.idle_dirty")
    if dirty:
        raise AssertionError("%s: %d handle-owned word(s) not at their idle value, first: %s" % (what, dirty, decode_idle(dev.getParam("debug.idle_first"))))


class Plan:
    """What the states need of the device, asked once: work bytes per state, image sizes, the shared scratch sizes."""

    def __init__(self, dev):
        lib = _lib.load()
        self.work, self.tmp0, self.tmp1 = {}, {}, {}
        for s in STATES:
            set_knobs(dev, s.knobs)
            wb, t0, t1 = ctypes.c_size_t(0), 0, 0
            if s.call in ("sort", "soa32", "top_byte", "msb"):
                tb = ctypes.c_size_t()
                bits = 32 if s.refused or s.call in ("top_byte", "msb") else s.bits
                check(lib.adlhip_radix_sort_scratch_bytes_for(dev._h, s.kind, s.n, bits, s.level, ctypes.byref(tb), ctypes.byref(wb)), "scratch_bytes_for")
                if s.call == "sort":
                    t0 = s.n * ESZ[s.kind]
                elif s.call == "soa32":
                    t0 = t1 = s.n * 4
                if s.name == "level-2-work-lean":
                    l1 = ctypes.c_size_t()
                    check(lib.adlhip_radix_sort_scratch_bytes_for(dev._h, s.kind, s.n, bits, 1, ctypes.byref(tb), ctypes.byref(l1)), "scratch_bytes_for")
                    assert wb.value < l1.value, "level 2 must be smaller than level 1 at this size: %d / %d" % (wb.value, l1.value)
            elif s.call == "soa":
                tk, tv = ctypes.c_size_t(), ctypes.c_size_t()
                check(lib.adlhip_radix_sort_soa_scratch_bytes(dev._h, 8, 16, s.n, s.bits, ctypes.byref(tk), ctypes.byref(tv), ctypes.byref(wb)), "soa scratch")
                t0, t1 = tk.value, tv.value
            elif s.call == "scan":
                check(lib.adlhip_scan_scratch_bytes(dev._h, s.n, ctypes.byref(wb)), "scan_scratch_bytes")
            self.work[s.name], self.tmp0[s.name], self.tmp1[s.name] = wb.value, t0, t1
        set_knobs(dev, {})
        self.tmp_half = align_up(max(self.tmp0.values()), 256)
        self.tmp_bytes = self.tmp_half + align_up(max(self.tmp1.values()), 256)
        self.work_bytes = align_up(max(self.work.values()), 256) + 256
        self.image_bytes = max(s.offsets()[1] for s in STATES)


class Bench:
    """One handle with what every call on it shares: d_tmp and d_work sized once for the largest state, `slots` data buffers,
    and a pristine device copy of every state's input image (restoring an input is one device-to-device copy)."""

    def __init__(self, slots, profiled=False):
        self.dev = DeviceUtils.allocate()
        self.profiled = profiled
        if profiled:
            self.dev.toggleProfiling(True)
        self.plan = Plan(self.dev)
        self.tmp = dmalloc(self.dev, self.plan.tmp_bytes)
        self.work = dmalloc(self.dev, self.plan.work_bytes)
        self.slots = [dmalloc(self.dev, self.plan.image_bytes) for _ in range(slots)]
        self.host = [np.empty(self.plan.image_bytes, np.uint8) for _ in range(slots)]
        self.totals = [np.zeros(1, np.uint32) for _ in range(slots)]
        self.pristine = {}
        self.allocs = [(self.tmp, self.plan.tmp_bytes), (self.work, self.plan.work_bytes)] + [(p, self.plan.image_bytes) for p in self.slots]
        lib = _lib.load()
        check(lib.adlhip_memset(self.dev._h, ctypes.c_void_p(self.tmp), 0xFF, self.plan.tmp_bytes), "memset")
        check(lib.adlhip_memset(self.dev._h, ctypes.c_void_p(self.work), 0xFF, self.plan.work_bytes), "memset")
        sync(self.dev)

    def close(self):
        lib = _lib.load()
        lib.adlhip_sync(self.dev._h)
        for p, nb in self.allocs + [(p, nb) for p, nb in self.pristine.values()]:
            check(lib.adlhip_free(self.dev._h, ctypes.c_void_p(p), nb), "adlhip_free")
        if self.profiled:
            self.dev.toggleProfiling(False)
        DeviceUtils.deallocate(self.dev)

    def restore(self, state, slot):
        """The state's input image into data buffer `slot` (stream-ordered)."""
        lib = _lib.load()
        if state.name not in self.pristine:
            img = state.image(1)
            p = dmalloc(self.dev, img.size)
            check(lib.adlhip_memcpy_h2d(self.dev._h, ctypes.c_void_p(p), img.ctypes.data_as(ctypes.c_void_p), img.size), "h2d")
            sync(self.dev)
            self.pristine[state.name] = (p, img.size)
        p, nb = self.pristine[state.name]
        check(lib.adlhip_memcpy_d2d(self.dev._h, ctypes.c_void_p(self.slots[slot]), ctypes.c_void_p(p), nb), "d2d")

    def enqueue(self, state, slot, knobs=None):
        """Sets the state's knobs and makes its call on data buffer `slot`; returns the call's status.  Nothing waits."""
        lib, h, s = _lib.load(), self.dev._h, state
        set_knobs(self.dev, s.knobs if knobs is None else knobs)
        offs, _ = s.offsets()
        at = lambda nm: ctypes.c_void_p(self.slots[slot] + offs[nm])
        tmp, tmp1, work = ctypes.c_void_p(self.tmp), ctypes.c_void_p(self.tmp + self.plan.tmp_half), ctypes.c_void_p(self.work)
        wb = self.plan.work[s.name]
        if s.call == "sort":
            fn = {U32: lib.adlhip_radix_sort_u32, KV32: lib.adlhip_radix_sort_kv32, U64: lib.adlhip_radix_sort_u64}[s.kind]
            if s.refused == "work+4":
                work = ctypes.c_void_p(self.work + 4)
            return fn(h, at("data"), tmp, work, wb, s.n, s.bits)
        if s.call == "soa32":
            return lib.adlhip_radix_sort_soa32(h, at("keys"), at("vals"), tmp, tmp1, work, wb, s.n, s.bits)
        if s.call == "soa":
            return lib.adlhip_radix_sort_soa(h, at("keys"), 8, at("vals"), 16, tmp, tmp1, work, wb, s.n, s.bits)
        if s.call == "scan":
            self.totals[slot][0] = 0xDEADBEEF
            return lib.adlhip_exclusive_scan_u32(h, at("dst"), at("src"), work, wb, s.n, self.totals[slot].ctypes.data_as(ctypes.c_void_p))
        if s.call == "top_byte":
            return lib.adlhip_partition_top_byte_u32(h, at("in"), at("out"), at("counts"), work, wb, s.n)
        if s.call == "msb":
            return lib.adlhip_partition_msb_kv32(h, at("in"), at("out"), at("counts"), work, wb, s.n, s.extra["buckets"])
        if s.call == "segsort":
            s.build()
            return lib.adlhip_segment_sort(h, s.kind, at("data"), at("seg_start"), s.extra["num_segments"], s.extra["bound"], s.bits)
        raise ValueError(s.call)

    def fetch(self, state, slot):
        """Enqueues the copy of data buffer `slot` to the host; valid once the stream has drained."""
        nb = state.offsets()[1]
        check(_lib.load().adlhip_memcpy_d2h(self.dev._h, self.host[slot].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.slots[slot]), nb), "d2h")

    def verify(self, state, slot, rc, what):
        if state.refused:
            assert rc != 0, "%s: %s was not refused" % (what, state.name)
        else:
            assert rc == 0, "%s: %s failed: %s" % (what, state.name, _lib_err())
        got = self.host[slot][:state.offsets()[1]]
        want = _want_image(state)
        if not np.array_equal(got, want):
            offs, _ = state.offsets()
            for nm, _, w in state.build():
                g = got[offs[nm]:offs[nm] + w.size]
                if not np.array_equal(g, w):
                    bad = np.flatnonzero(g != w)
                    raise AssertionError("%s: %s: array '%s' differs from the host reference in %d bytes, first at byte %d (element %d)" % (
                        what, state.name, nm, bad.size, bad[0], bad[0] // max(1, ESZ.get(state.kind, 4))))
            raise AssertionError("%s: %s: bytes between the arrays changed" % (what, state.name))
        if state.call == "scan":
            assert int(self.totals[slot][0]) == state.extra["total"], "%s: scan total" % what


_WANT = {}


def _want_image(state):
    if state.name not in _WANT:
        _WANT[state.name] = state.image(2)
    return _WANT[state.name]


# calibration: state name -> (labels, (net runs, net counting)) of the state alone on a fresh handle
CALIB = {}


def calibrate(state):
    """Runs the state alone, synced and profiled, on a fresh handle; asserts its claims; records labels and net delta."""
    if state.name in CALIB:
        return CALIB[state.name]
    b = Bench(1, profiled=True)
    try:
        dev = b.dev
        assert_idle(dev, "fresh handle")
        b.restore(state, 0)
        sync(dev)
        dev.profile(reset=True)
        r0, c0 = net_stats(dev)
        rc = b.enqueue(state, 0)
        sync(dev)
        labels = set(dev.profile(reset=True))
        r1, c1 = net_stats(dev)
        net = (r1 - r0, c1 - c0)
        b.fetch(state, 0)
        sync(dev)
        print("calibration %-34s work %10d  net %s  labels %s" % (state.name, b.plan.work[state.name], net, sorted(labels)))
        b.verify(state, 0, rc, "calibration")
        if state.refused:
            assert not labels, (state.name, labels)
        assert state.labels <= labels, "%s: claimed kernels not launched: %s (launched: %s)" % (state.name, sorted(state.labels - labels), sorted(labels))
        if state.net == NET_NONE:
            assert net == (0, 0), "%s: the safety net ran on a friendly state: %s" % (state.name, net)
        elif state.net == NET_LSD:
            assert net[0] >= 1 and net[1] == 0, "%s: claimed a net that runs LSD passes, got (runs, counting) = %s" % (state.name, net)
        else:
            assert net[0] >= 1 and net[1] > 0, "%s: claimed a net that sorts by counting, got (runs, counting) = %s" % (state.name, net)
        assert_idle(dev, "calibration of %s" % state.name)
        CALIB[state.name] = (labels, net)
        _dump_report()
        return CALIB[state.name]
    finally:
        b.close()


def _dump_report():
    path = os.environ.get("ADLHIP_SEQUENCE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({k: {"labels": sorted(v[0]), "net": v[1]} for k, v in CALIB.items()}, f, indent=1)


def expected_net(states):
    runs = sum(calibrate(s)[1][0] for s in states)
    counting = sum(calibrate(s)[1][1] for s in states)
    return runs, counting


def run_batch(bench, states, what, drain=sync, results_only=(), knobs_for=None):
    """Restores the inputs, queues the calls back to back without waiting, drains, and makes the three assertions."""
    dev = bench.dev
    for i, s in enumerate(states):
        bench.restore(s, i)
    drain(dev)
    r0, c0 = net_stats(dev)
    rcs = [bench.enqueue(s, i, knobs_for(i, s) if knobs_for else None) for i, s in enumerate(states)]
    drain(dev)                                     # must succeed: nothing raised the fault word
    for i, s in enumerate(states):
        bench.fetch(s, i)
    drain(dev)
    names = " -> ".join(s.name for s in states)
    for i, s in enumerate(states):
        bench.verify(s, i, rcs[i], "%s [%s], call %d" % (what, names, i))
    r1, c1 = net_stats(dev)
    counted = [s for i, s in enumerate(states) if i not in results_only]
    if len(counted) == len(states):
        assert (r1 - r0, c1 - c0) == expected_net(states), "%s [%s]: the net ran (runs, counting) = %s, the same calls on fresh handles %s" % (
            what, names, (r1 - r0, c1 - c0), expected_net(states))
    assert_idle(dev, "%s [%s]" % (what, names))


@pytest.fixture(scope="module")
def bench():
    b = Bench(8)
    yield b
    b.close()


@pytest.fixture(autouse=True)
def _default_knobs(request):
    yield
    if "bench" in request.fixturenames:
        set_knobs(request.getfixturevalue("bench").dev, {})


# ---------------------------------------------------------------------------------------------
# 1. the checker sees one flipped bit, in every region
# ---------------------------------------------------------------------------------------------
def test_idle_checker_sees_one_flipped_bit_in_every_region():
    dev = DeviceUtils.allocate()
    try:
        assert dev.getParam("debug.idle_dirty") == 0 and dev.getParam("debug.idle_first") == 0
        # an idle-valued word of each area: a second-pass cursor, the sample's AND word (idle: all ones), a slice histogram
        # word, the two-launch form's reader counter, the dictionary block's padding, mid_prep_kernel's arrival counter
        for region, word in ((1, 8192 + 4711), (1, MSD2_FLAG + 10), (1, MSD2_FLAG + 12), (2, 777), (2, MID_STATE + 8193), (3, 2), (4, 12)):
            code = (region << 24) | word
            dev.setParam("debug.idle_poke", code)
            assert dev.getParam("debug.idle_dirty") == 1, decode_idle(code)
            assert dev.getParam("debug.idle_first") == code, (decode_idle(dev.getParam("debug.idle_first")), decode_idle(code))
            dev.setParam("debug.idle_poke", code)
            assert dev.getParam("debug.idle_dirty") == 0 and dev.getParam("debug.idle_first") == 0, decode_idle(code)
        # words that are reset on entry or free-running do not count: the net's barrier counter, its run counter
        for word in (MSD2_FLAG + 2, MSD2_FLAG + 16):
            dev.setParam("debug.idle_poke", (1 << 24) | word)
            assert dev.getParam("debug.idle_dirty") == 0
            dev.setParam("debug.idle_poke", (1 << 24) | word)
        for bad in (0, (5 << 24), (4 << 24) | 16, (1 << 24) | (MSD2_FLAG + 64)):
            assert _lib.load().adlhip_set_param(dev._h, b"debug.idle_poke", bad) != 0 and _lib_err()
        sync(dev)
    finally:
        DeviceUtils.deallocate(dev)


# ---------------------------------------------------------------------------------------------
# 2. calibration: every state alone on a fresh handle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES, ids=[s.name for s in STATES])
def test_calibration_every_state_alone_on_a_fresh_handle(state):
    calibrate(state)


# ---------------------------------------------------------------------------------------------
# 3. every ordered pair on one long-lived handle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", STATES, ids=[s.name for s in STATES])
def test_every_state_followed_by_every_state(bench, first):
    for second in STATES:
        run_batch(bench, [first, second], "pair")


# ---------------------------------------------------------------------------------------------
# 4. seeded walks
# ---------------------------------------------------------------------------------------------
WALK_STEPS, WALK_GROUP = 48, 8


def _event_drain(dev):
    """Waits for the handle's stream as a foreign owner of the stream would (an event), then asks for faults without blocking."""
    lib = _lib.load()
    ev = ctypes.c_void_p()
    check(lib.adlhip_event_create(dev._h, ctypes.byref(ev)), "event_create")
    try:
        check(lib.adlhip_event_record(dev._h, ev), "event_record")
        check(lib.adlhip_event_synchronize(dev._h, ev), "event_synchronize")
    finally:
        lib.adlhip_event_destroy(dev._h, ev)
    assert lib.adlhip_fault_check(dev._h) == 0, "adlhip_fault_check reported: %s" % _lib_err()


@pytest.mark.parametrize("seed", [11, 12])
def test_seeded_walk_over_all_states(bench, seed):
    rng = np.random.default_rng(seed)
    # every state at least once, then random ones
    order = list(rng.permutation(len(STATES))) + list(rng.integers(0, len(STATES), max(0, WALK_STEPS - len(STATES))))
    while len(order) % WALK_GROUP:
        order.append(int(rng.integers(0, len(STATES))))
    assert len(order) >= WALK_STEPS
    for g in range(0, len(order), WALK_GROUP):
        run_batch(bench, [STATES[i] for i in order[g:g + WALK_GROUP]], "walk %d, calls %d..%d" % (seed, g, g + WALK_GROUP - 1))


def test_seeded_walk_with_the_mid_size_form_left_to_the_host(bench):
    """"sort.mid" = 1: the host picks the mid-size form from pinned reports that may be a sort or two old (choose_mid_form), so
    friendly and skewed mid-size inputs in turns change the form of later ones.  Only speed may depend on that: for the mid-size
    steps the results are asserted, for the others the net's count too; the idle state after every group."""
    rng = np.random.default_rng(13)
    others = [s for s in STATES if s.name not in MID_STATES]
    order = []
    for i in range(WALK_STEPS):
        order.append(STATE_BY_NAME[MID_STATES[(i // 2) % 4]] if i % 2 == 0 else others[int(rng.integers(0, len(others)))])
    mid_knobs = lambda i, s: dict(s.knobs, **{"sort.mid": 1}) if s.name in MID_STATES else s.knobs
    for g in range(0, WALK_STEPS, WALK_GROUP):
        group = order[g:g + WALK_GROUP]
        dev = bench.dev
        r0, c0 = net_stats(dev)
        run_batch(bench, group, "mid walk, calls %d..%d" % (g, g + WALK_GROUP - 1), knobs_for=mid_knobs,
                  results_only={i for i, s in enumerate(group) if s.name in MID_STATES})
        r1, c1 = net_stats(dev)
        # no mid-size input reaches the large sort whatever form it took: the group's net count is that of its other calls
        assert (r1 - r0, c1 - c0) == expected_net([s for s in group if s.name not in MID_STATES]), (g, (r1 - r0, c1 - c0))


def test_seeded_walk_drained_by_fault_checks(bench):
    """The same walk on a handle whose stream someone else waits for: an event instead of adlhip_sync, adlhip_fault_check between
    the groups (tests/test_gpu_parity.py test_fault_check_is_stream_ordered_and_reports_once)."""
    rng = np.random.default_rng(14)
    order = [int(i) for i in rng.integers(0, len(STATES), WALK_STEPS)]
    for g in range(0, WALK_STEPS, WALK_GROUP):
        run_batch(bench, [STATES[i] for i in order[g:g + WALK_GROUP]], "fault-check walk, calls %d..%d" % (g, g + WALK_GROUP - 1), drain=_event_drain)
    sync(bench.dev)


# ---------------------------------------------------------------------------------------------
# 5. the same input is treated the same way on the handle that has seen everything
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", [s for s in STATES if s.large], ids=[s.name for s in STATES if s.large])
def test_large_sort_takes_the_same_path_after_everything_else(bench, state):
    labels0, net0 = calibrate(state)
    dev = bench.dev
    dev.toggleProfiling(True)
    try:
        bench.restore(state, 0)
        sync(dev)
        dev.profile(reset=True)
        r0, c0 = net_stats(dev)
        rc = bench.enqueue(state, 0)
        sync(dev)
        labels = set(dev.profile(reset=True))
        r1, c1 = net_stats(dev)
    finally:
        dev.toggleProfiling(False)
    bench.fetch(state, 0)
    sync(dev)
    bench.verify(state, 0, rc, "after everything else")
    assert labels == labels0, "%s: kernels differ from the fresh handle's: only here %s, only there %s" % (
        state.name, sorted(labels - labels0), sorted(labels0 - labels))
    assert (r1 - r0, c1 - c0) == net0, (state.name, (r1 - r0, c1 - c0), net0)
    assert_idle(dev, state.name)


# ---------------------------------------------------------------------------------------------
# 6. sorts queued behind a call that raises the software fault word
# ---------------------------------------------------------------------------------------------
def test_sorts_queued_behind_a_reported_fault_word(bench):
    """adlhip_segment_sort with one segment of cap + 1 keys leaves the segment as it is and raises the library's fault word (the
    kernel returns normally; tests/test_gpu_parity.py test_fault_check_is_stream_ordered_and_reports_once makes the same call).  A
    friendly large sort and a mid-size sort queued behind it are exact, the sync reports the fault once, and the handle is idle."""
    lib, dev = _lib.load(), bench.dev
    cap = 4096
    starts = np.array([0, cap + 1], dtype=np.uint32)
    seg = dmalloc(dev, 256)
    data = dmalloc(dev, 4 * (cap + 1))
    try:
        check(lib.adlhip_memcpy_h2d(dev._h, ctypes.c_void_p(seg), starts.ctypes.data_as(ctypes.c_void_p), 8), "h2d")
        check(lib.adlhip_memset(dev._h, ctypes.c_void_p(data), 0, 4 * (cap + 1)), "memset")
        large, mid = STATE_BY_NAME["cursor-friendly"], STATE_BY_NAME["mid2-friendly"]
        bench.restore(large, 0)
        bench.restore(mid, 1)
        sync(dev)
        r0, c0 = net_stats(dev)
        check(lib.adlhip_segment_sort(dev._h, 0, ctypes.c_void_p(data), ctypes.c_void_p(seg), 1, cap, 8), "segment_sort")
        rc0 = bench.enqueue(large, 0)
        rc1 = bench.enqueue(mid, 1)
        assert lib.adlhip_sync(dev._h) != 0, "the fault word was not reported"
        assert "fault" in _lib_err(), _lib_err()
        sync(dev)                                  # reported once
        bench.fetch(large, 0)
        bench.fetch(mid, 1)
        sync(dev)
        bench.verify(large, 0, rc0, "behind a fault word")
        bench.verify(mid, 1, rc1, "behind a fault word")
        r1, c1 = net_stats(dev)
        assert (r1 - r0, c1 - c0) == (0, 0), (r1 - r0, c1 - c0)
        assert_idle(dev, "behind a fault word")
    finally:
        lib.adlhip_sync(dev._h)
        check(lib.adlhip_free(dev._h, ctypes.c_void_p(seg), 256), "adlhip_free")
        check(lib.adlhip_free(dev._h, ctypes.c_void_p(data), 4 * (cap + 1)), "adlhip_free")
