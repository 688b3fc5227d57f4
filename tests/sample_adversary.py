"""Keys built against the large sort's own samples (plain numpy, no GPU; tests/test_sample_adversary.py checks this module on the
CPU, tests/test_gpu_sample_adversary.py drives the device with it).

The large sort decides how to sort from three samples of its input:

  S   2048 keys   hybrid_kernels.hpp sample_position (msd2_sample_kernel, msd2s_prep_kernel): the digits' place (msd2_placement) and
                  the per-wave repeat count that is compared with adlhip.hip sample_dup_threshold, kDictMinRepeats, kBigMinRepeats
  P  16384 keys   hybrid_kernels.hpp probe_sample_index (dict_sample_build, dict_sample_build_pair_keys): the net's dictionary of at
                  most 256 values
  B  65536 keys   dict_big_kernels.hpp big_sample_index (big_dict_sample): the dictionary of at most 4096 values, u32 keys only

All three position functions are integer arithmetic on (k, n).  positions_S / positions_P / positions_B are their twins -- the same
constants, the same 32- and 64-bit wrap-around -- so that a test chooses separately what each sample reads and what the other 97 % of
the array holds.  A CHANGE OF A CONSTANT IN ONE OF THE DEVICE FUNCTIONS MUST BE FOLLOWED HERE; the controls of
tests/test_gpu_sample_adversary.py fail otherwise.
"""
import math

import numpy as np

S_SAMPLES, P_SAMPLES, B_SAMPLES = 2048, 16384, 65536
S_WAVES, S_PER_WAVE = 16, 128          # wave w reads samples 128 w .. 128 w + 127, two per lane (sample_accumulate)
DICT_MAX, DICT_MIN_REPEATS = 256, 256  # dict_build.hpp kDictMax, kDictMinRepeats
BIG_MAX, BIG_MIN_REPEATS = 4096, 18    # dict_big_kernels.hpp kBigMax, kBigMinRepeats
BIG_MIN_N = 1 << 20                    # net_sort: the big dictionary is tried from here
M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------
def _scramble32(k):
    """h of sample_position / big_sample_index: uint32 arithmetic, carried out in uint64 and masked"""
    h = (k * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(13)
    return h


def positions_S(n):
    """sample_position(k, n) for k < 2048: inside [k n / 2048, (k + 1) n / 2048), no clamp on the device (hi <= n)"""
    k = np.arange(S_SAMPLES, dtype=np.uint64)
    lo, hi = k * np.uint64(n) // np.uint64(S_SAMPLES), (k + np.uint64(1)) * np.uint64(n) // np.uint64(S_SAMPLES)
    return (lo + ((_scramble32(k) * (hi - lo)) >> np.uint64(32))).astype(np.int64)


def positions_P(n):
    """probe_sample_index(k, n) for k < 16384 (n >= 16384), the `at >= n` clamp included"""
    assert n >= P_SAMPLES
    k = np.arange(P_SAMPLES, dtype=np.uint64)
    cell = np.uint64(n >> 14)
    with np.errstate(over="ignore"):
        hash24 = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)       # the product wraps at 2^64 as on the device
    jit = (hash24 * cell) >> np.uint64(24)
    at = k * np.uint64(n) // np.uint64(P_SAMPLES) + jit
    return np.minimum(at, np.uint64(n - 1)).astype(np.int64)


def positions_B(n):
    """big_sample_index(k, n) for k < 65536 (n >= 2^20), no clamp on the device"""
    assert n >= BIG_MIN_N
    k = np.arange(B_SAMPLES, dtype=np.uint64)
    lo, hi = (k * np.uint64(n)) >> np.uint64(16), ((k + np.uint64(1)) * np.uint64(n)) >> np.uint64(16)
    return (lo + ((_scramble32(k) * (hi - lo)) >> np.uint64(32))).astype(np.int64)


POSITIONS = {"S": positions_S, "P": positions_P, "B": positions_B}
CELLS = {"S": S_SAMPLES, "P": P_SAMPLES, "B": B_SAMPLES}


def cell_bounds(which, n):
    """[lo, hi) of every sample's cell, as the device code states them (B: shifts, S and P: divisions)"""
    c = CELLS[which]
    k = np.arange(c, dtype=np.uint64)
    lo, hi = k * np.uint64(n) // np.uint64(c), (k + np.uint64(1)) * np.uint64(n) // np.uint64(c)
    return lo.astype(np.int64), hi.astype(np.int64)


def union_positions(n):
    return np.unique(np.concatenate([positions_S(n), positions_P(n), positions_B(n)]))


def sample_dup_threshold(n):
    """adlhip.hip sample_dup_threshold"""
    s, d = 128.0, max(1.0, n / 3072.0)
    return int(max(4.0, 0.8 * 16.0 * (s - d * (1.0 - math.exp(-s / d)))))


# ---------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------
def _mix(x, width):
    """A bijection of the `width`-bit integers (the finalisers of MurmurHash3): distinct arguments give distinct keys."""
    x = x.astype(np.uint64)
    with np.errstate(over="ignore"):
        if width == 32:
            x &= M32
            x ^= x >> np.uint64(16)
            x = (x * np.uint64(0x85EBCA6B)) & M32
            x ^= x >> np.uint64(13)
            x = (x * np.uint64(0xC2B2AE35)) & M32
            x ^= x >> np.uint64(16)
            return x
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
        return x


def value_table(count, width, seed):
    """`count` distinct key values; a longer table of the same seed starts with the shorter one"""
    return _mix(np.arange(count, dtype=np.uint64) + np.uint64(0x51ED27 + 7919 * seed), width)


def wave_keys(width):
    """16 keys, one per wave of S, whose top four bits -- of the whole key and of its low 24 bits -- are the wave's number: they fall
    into 16 different buckets and segments"""
    w = np.arange(S_WAVES, dtype=np.uint64)
    if width == 32:
        return (w * np.uint64(0x10101010)) | np.uint64(0x0A0B0C0D)
    return (w * np.uint64(0x1010101010101010)) | np.uint64(0x0A0B0C0D0A0B0C0D)


def _fill(recipe, at, width, seed, which):
    """keys for the positions `at` (ascending, int64).  Recipes:
    ("uniform",)        distinct random keys: a bijection of the position, so distinct over the whole array too
    ("one", K)          the key K
    ("values", d)       drawn from the first d values of value_table(seed)
    ("below", b)        random keys below 2^b
    ("high_only",)      random in bits 24 and up, one constant in the 24 bits below
    ("by_wave",)        S only: sample k holds wave_keys()[k // 128]"""
    rng = np.random.default_rng([seed, {"S": 1, "P": 2, "B": 3, "rest": 4}[which]])
    kind = recipe[0]
    if kind == "uniform":
        return _mix(at.astype(np.uint64) + np.uint64(0x9E3779B1 * (seed + 1)), width)
    if kind == "one":
        return np.full(at.size, recipe[1], np.uint64)
    if kind == "values":
        return value_table(recipe[1], width, seed)[rng.integers(0, recipe[1], at.size)]
    if kind == "below":
        return rng.integers(0, 1 << recipe[1], at.size, dtype=np.uint64)
    if kind == "high_only":
        hi = _mix(at.astype(np.uint64) + np.uint64(77), width) & ~np.uint64(0xFFFFFF)
        return hi | np.uint64(0x5A5A5A)
    if kind == "by_wave":
        assert which == "S" and at.size == S_SAMPLES
        return wave_keys(width)[np.arange(S_SAMPLES) // S_PER_WAVE]
    raise ValueError(recipe)


def build(kind, n, seen, rest, seed, shift=0, extra=()):
    """An array of n u32 keys, u64 keys or kv32 pairs ({key, value = the element's index}: the low dword is the key).

    seen    {"S" | "P" | "B": recipe}: what those samples read.  Where the sets overlap S wins over P and P over B.
    rest    the recipe of every position not named in `seen`
    shift   the seen keys are written `shift` elements behind the sampled positions (the controls' "one element off"; the last
            element stays inside the array)
    extra   [(positions, keys)] written last"""
    width = 64 if kind == "u64" else 32
    keys = _fill(rest, np.arange(n, dtype=np.int64), width, seed, "rest")
    for which in ("B", "P", "S"):
        if which in seen:
            at = POSITIONS[which](n)
            keys[np.minimum(at + shift, n - 1)] = _fill(seen[which], at, width, seed, which)
    for at, vals in extra:
        keys[at] = vals
    if kind == "u32":
        return keys.astype(np.uint32)
    if kind == "u64":
        return keys
    assert kind == "kv32", kind
    return (keys & M32) | (np.arange(n, dtype=np.uint64) << np.uint64(32))


def keys_of(kind, arr):
    return (arr & M32).astype(np.uint32) if kind == "kv32" else arr


def rare_sites(which, n, count):
    """About `count` sampled positions of set `which`, taken with a stride over its cells, the first and the last cell among them,
    each with a neighbour (one element behind, else one before) that NO sample reads: (positions, neighbours).  Cells without such a
    neighbour are left out."""
    at = POSITIONS[which](n)
    cells = np.unique(np.round(np.linspace(0, at.size - 1, count)).astype(np.int64))
    u = union_positions(n)
    on = at[cells]
    free = lambda p: (p >= 0) & (p < n) & ~np.isin(p, u)
    off = np.where(free(on + 1), on + 1, on - 1)
    ok = free(off)
    return on[ok], off[ok]


# ---------------------------------------------------------------------------------------------
# what the samples observe
# ---------------------------------------------------------------------------------------------
class Seen:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "Seen(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.__dict__.items()))


def sees(keys, n, sort_bits=None):
    """What each sample observes of `keys` (u32 or u64 keys; the key dwords of pairs):
    distinct_P, distinct_B   values among the 16384 / 65536 probes (whole keys: the dictionaries serve whole-key sorts only); B is
                             None where the big dictionary does not exist (u64 keys, n < 2^20)
    diff, top                OR ^ AND of S after the sort-bits mask, and `top` as msd2_placement / msd2s_prep_kernel compute it
    repeats                  the sum over the 16 waves of S of the samples that repeat an earlier one of their wave
    threshold                sample_dup_threshold(n)"""
    assert keys.size == n
    width = 8 * keys.dtype.itemsize
    bits = width if sort_bits is None else sort_bits
    mask = (1 << bits) - 1
    s = keys[positions_S(n)].astype(np.uint64) & np.uint64(mask)
    diff = int(np.bitwise_or.reduce(s)) ^ int(np.bitwise_and.reduce(s))
    top = max(16, diff.bit_length())
    repeats = sum(S_PER_WAVE - np.unique(s[w * S_PER_WAVE:(w + 1) * S_PER_WAVE]).size for w in range(S_WAVES))
    big = width == 32 and n >= BIG_MIN_N
    return Seen(distinct_P=int(np.unique(keys[positions_P(n)]).size), distinct_B=int(np.unique(keys[positions_B(n)]).size) if big else None,
                diff=diff, top=top, repeats=int(repeats), threshold=sample_dup_threshold(n))


# ---------------------------------------------------------------------------------------------
# the cases (tests/test_gpu_sample_adversary.py runs them; tests/test_sample_adversary.py asserts the `premise` of every row)
# ---------------------------------------------------------------------------------------------
K_ONE = {32: 0x6B8B4567, 64: 0x6B8B4567327B23C6}
FULL = "full"   # `top` = the sorted width


class Case:
    def __init__(self, name, seen, rest, premise, why, only=None):
        self.name, self.seen, self.rest, self.premise, self.why, self.only = name, seen, rest, premise, why, only

    def applies(self, kind, bits):
        if self.only == "24 bits":
            return bits == 24
        if self.only == "pairs":
            return kind == "kv32"
        return True

    def recipes(self, width):
        fix = lambda r: ("one", K_ONE[width]) if r == ("one",) else r
        return {k: fix(v) for k, v in self.seen.items()}, fix(self.rest)

    def build(self, kind, n, seed):
        seen, rest = self.recipes(64 if kind == "u64" else 32)
        return build(kind, n, seen, rest, seed)


def _all(recipe):
    return {"S": recipe, "P": recipe, "B": recipe}


# Every row ends in the net's LSD passes, (net runs, counting) = (1, 0); `why` derives it from the code.  The dictionaries exist
# for whole-key sorts only (adlhip.hip msd2_sort, msd2s_sort net_dict): the small one for u32, u64 and pair keys, the big one for
# u32 keys; the 24-bit sort and the SoA sort go from the net's entry straight to the LSD passes.
# premise: what sees() must report -- repeats as (lowest, highest), "thr" = sample_dup_threshold(n).
CASES = [
    Case("1-uniform-seen-one-key-rest", _all(("uniform",)), ("one",),
         dict(repeats=(0, 0), top=FULL, P=(DICT_MAX + 1, None), B=(BIG_MAX + 1, None)),
         "no repeats: the passes run; the sampled keys differ in the top bit, so the first digit is the top byte of the sorted bits and "
         "97 % of the keys -- one value -- meet in one bucket, whose slab holds 1.5 n / 256 + 4096: overflow flag, net.  0 repeats < "
         "kBigMinRepeats < kDictMinRepeats: no dictionary is tried, LSD passes."),
    Case("2-one-key-seen-uniform-rest", _all(("one",)), ("uniform",),
         dict(repeats=(2032, 2032), top=16, P=(1, 1), B=(1, 1)),
         "16 x 127 repeats >= the threshold: every pass leaves at its first instruction (large_sort_gave_up) and the offsets kernel "
         "enters the net with top = 16 and a prefix of that one key in the sample words.  >= kDictMinRepeats: dict_sample_build "
         "makes a dictionary of 1 value, dict_count_range raises `miss` in nearly every workgroup (pairs: coop_dict_pair_sort returns "
         "0 before it has written anything to `data`); u32 keys: the big dictionary, 1 value, `miss` again; LSD passes."),
    Case("3-S-one-key-P-B-uniform", {"S": ("one",), "P": ("uniform",), "B": ("uniform",)}, ("uniform",),
         dict(repeats=(2032, 2032), top=16, P=(DICT_MAX + 1, None), B=(BIG_MAX + 1, None)),
         "the passes give up as in case 2; P shows more than 256 values, dict_build leaves n_values = 0 and the count phase is "
         "skipped; u32 keys: B shows more than 4096, big_dict_build leaves n_values = 0; LSD passes."),
    Case("4-256-values-seen-300-rest", _all(("values", 256)), ("values", 300),
         dict(repeats=(DICT_MIN_REPEATS, None), P=(256, 256), B=(256, 256)),
         "256 equally likely values repeat ~436 times in S: >= the threshold, so the passes give up at once and no pass overflow "
         "interleaves with the dictionaries; >= kDictMinRepeats: the small dictionary is built complete for what P shows (256 values) "
         "and the 44 others raise `miss`; u32 keys: the big dictionary is built of the same 256 values, `miss` again; LSD passes."),
    Case("5-below-2^20-seen-full-width-rest", _all(("below", 20)), ("uniform",),
         dict(repeats=(0, BIG_MIN_REPEATS - 1), top=20, P=(DICT_MAX + 1, None), B=(BIG_MAX + 1, None)),
         "fewer repeats than the threshold: the passes run with top = 20 and prefix 0; pass 1 compares every key's bits from 20 up "
         "with the prefix and nearly every key fails: overflow flag in the first tiles, net.  Fewer than kBigMinRepeats: LSD passes."),
    Case("6-full-width-seen-below-2^16-rest", _all(("uniform",)), ("below", 16),
         dict(repeats=(0, 0), top=FULL, P=(DICT_MAX + 1, None), B=(BIG_MAX + 1, None)),
         "no repeats, top = the sorted width: 97 % of the keys have first digit 0 and overflow bucket 0's slab: net, no dictionary, "
         "LSD passes -- for pairs with ~46 copies of every key below 2^16, whose order the passes must keep."),
    Case("7-seen-differ-above-bit-24-only", _all(("high_only",)), ("uniform",),
         dict(repeats=(2032, 2032), top=16, whole_diff=True),
         "msd2s_prep_kernel masks the samples to the 24 sorted bits: constant, 16 x 127 repeats, the passes give up as in case 2.  A "
         "sort on part of the key has no dictionary (net_dict = nullptr): LSD passes on 24 bits.", only="24 bits"),
    Case("8-16-key-values-seen-uniform-rest", _all(("values", 16)), ("uniform",),
         dict(repeats=(DICT_MIN_REPEATS, None), P=(16, 16)),
         "16 values: 16 x 112 repeats, the passes give up; dict_sample_build_pair_keys makes a dictionary of 16 key values, "
         "coop_dict_pair_sort's count phase raises `miss` and returns 0 with `data` untouched; the LSD passes sort the pairs and must "
         "keep equal keys in input order.", only="pairs"),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def check_premise(case, keys, n, bits):
    """asserts that sees() reports what the row claims; returns the Seen"""
    width = 8 * keys.dtype.itemsize
    s = sees(keys, n, bits)
    p = case.premise

    def within(name, got, rng):
        lo, hi = rng
        assert got >= lo and (hi is None or got <= hi), "%s: %s = %r, the row claims [%r, %r]; %r" % (case.name, name, got, lo, hi, s)

    within("repeats", s.repeats, p["repeats"])
    if p["repeats"][0] > 0:
        assert s.repeats >= s.threshold, (case.name, s)
    else:
        assert s.repeats < s.threshold and s.repeats < BIG_MIN_REPEATS, (case.name, s)
    if "top" in p:
        assert s.top == (bits if p["top"] == FULL else p["top"]), "%s: top = %d; %r" % (case.name, s.top, s)
    if "P" in p and bits == width:
        within("distinct_P", s.distinct_P, p["P"])
    if "B" in p and bits == width and s.distinct_B is not None:
        within("distinct_B", s.distinct_B, p["B"])
    if p.get("whole_diff"):
        assert sees(keys, n).diff != 0, "%s: the sampled keys do not differ above the sorted bits" % case.name
    return s
