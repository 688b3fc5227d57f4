"""The sort's fallback configurations as the typed primitives meet them: the configurations, the sizes, the shapes of rows and segments
and the rules that tell from a profile's launch labels which form of the inner sort ran (plain Python and numpy, no GPU;
tests/test_typed_fallbacks.py checks this module on the CPU, tests/test_gpu_typed_fallbacks.py uses it).

Nine typed entry points run the unsigned radix sort beneath them (primitives.hip: sort_elements, typed_index_sort,
adlhip_radix_sort_soa32).  The library leaves the configuration an unpartitioned MI355X picks by itself in two cases -- a partition
that cannot keep 256 workgroups resident, a device whose LDS-order self-test failed -- and the user can leave it through "sort.algo"
and "sort.digit_bits".  CONFIGS names the five configurations; the constants are those of adlhip.hip and large_plan.hpp.

The inner sorts of one call are described by Sort(kind, n): kind "pairs" is the stable {key dword, index} pair sort of
typed_index_sort, "keys32" / "keys64" the whole-key sort of adlhip_sort_keys_typed, "positions" the u32 sort of the k positions the
top-k selection found (whole u32 keys that all lie below 2^24: never friendly to the mid-size form, whatever the caller's keys are),
"soa" the (row or segment or class, position) sort of the flat paths and of the segment kernel's plan.  check_labels() states what each
configuration must show for them.
"""
from collections import namedtuple

import numpy as np

# adlhip.hip, large_plan.hpp
SMALL_MAX = 16384                 # kSmallMax: one workgroup sorts up to here
MID_MIN_U32 = 8192                # kMidMinU32
MID_MAX_E64 = 1 << 20             # kMidMaxE64 = kMsd2sAutoMin: pairs leave the mid-size form for the large stable form above
MID_MAX_U32 = 2 << 20             # kMidMaxU32 = kMsd2AutoMin: whole u32 keys leave the mid-size form for the large form above

# name, knobs in the order they are set
CONFIGS = [
    ("default", []),
    ("rank0", [("sort.rank", 0)]),                                           # the LDS-order self-test failed
    ("small_partition", [("debug.resident_wgs", 120)]),                      # fewer than 256 resident workgroups
    ("one_sweep", [("sort.algo", 0)]),                                       # per-digit look-back passes
    ("three_kernel_4bit", [("sort.algo", 1), ("sort.digit_bits", 4)]),       # the reference's pass structure
]
CONFIG_NAMES = [c[0] for c in CONFIGS]
KNOBS_OF = dict(CONFIGS)
# what puts a knob back; "sort.rank" goes back to what the device's self-test allows ("sort.lds_ordered"), "debug.resident_wgs" = 0
# restores the device's own answer
RESTORE = {"sort.rank": "sort.lds_ordered", "debug.resident_wgs": 0, "sort.algo": -1, "sort.digit_bits": 8}

# the smallest sizes that still tell the forms apart
PAIR_RUNGS = [20011, 300007, (1 << 20) + 4099]     # just past the one-workgroup sort, the mid-size range, the large stable form
KEY_RUNGS = {4: [300007, (1 << 21) + 4099], 8: [20011, 300007]}   # adlhip_sort_keys_typed sorts whole keys
# (type, case) of typed_shapes.shape
CASES = [("f64", "normal"), ("f32", "nan30"), ("i64", "ids"), ("i64", "uniform_pm1000"), ("f64", "normal_specials")]
CASE_IDS = ["%s-%s" % c for c in CASES]
SEED = 11

# rows x cols at a row stride whose totals sit on the rungs; no column count is a power of two, and the strided shapes start their
# rows at odd elements
ROW_SHAPES = [(7, 2861, 2861), (37, 8109, 8111), (131, 8037, 8037)]
# top-k along rows by the per-row loop: every row is one inner sort, so the COLUMNS sit on the rungs
TOPK_ROW_SHAPES = [(3, 20011, 20013), (2, 300007, 300007), (2, (1 << 20) + 4099, (1 << 20) + 4101)]
# the segment kernel's plan sorts (class, segment id) pairs: this many segments of 0 .. 52 keys
PLAN_SEGMENTS = 20011


Sort = namedtuple("Sort", "kind n")


def pair_form(n):
    """the form the stable pair sort of n pairs takes by default: "small", "mid" or "large\""""
    return "small" if n <= SMALL_MAX else ("mid" if n <= MID_MAX_E64 else "large")


def keys_form(width, n):
    """the same for whole keys of `width` bytes: u64 keys have no mid-size form and take the large sort from the one-workgroup limit"""
    if n <= SMALL_MAX:
        return "small"
    if width == 8:
        return "large"
    return "mid" if n <= MID_MAX_U32 else "large"


def form_of(sort):
    if sort.kind == "pairs":
        return pair_form(sort.n)
    if sort.kind == "soa":
        return "passes"   # adlhip_radix_sort_soa32 on fewer than 16 bits: the per-digit passes whatever n is
    return keys_form(8 if sort.kind == "keys64" else 4, sort.n)


def topk_ks(n):
    """one k at most n / 8 (the selection by default) and one above (the full argsort) that stays on the rung of n, so that the
    selection's k-element finish meets the size class too"""
    return [n // 8 - 3, n - 5]


def segment_lengths(n, segments, seed, longest=None):
    """`segments` lengths that sum to n: they vary, about one in six is empty -- the first, the last and a run of three among them --
    and none exceeds `longest` when given"""
    rng = np.random.default_rng([seed, n, segments])
    w = rng.random(segments) ** 2
    w[rng.random(segments) < 1 / 6] = 0
    w[0] = w[-1] = 0
    mid = segments // 2
    w[mid:mid + 3] = 0
    live = np.flatnonzero(w)
    lens = np.zeros(segments, np.int64)
    lens[live] = np.floor(w[live] / w[live].sum() * (n - live.size)).astype(np.int64) + 1   # every live segment holds a key
    if longest is not None:
        lens = np.minimum(lens, longest)
    short = n - int(lens.sum())
    i = 0
    while short > 0:   # hand the rest out, one key at a time, to live segments with room
        s = live[i % live.size]
        if longest is None or lens[s] < longest:
            lens[s] += 1
            short -= 1
        i += 1
    assert lens.sum() == n and (lens == 0).sum() >= 5
    return [int(x) for x in lens]


# ---------------------------------------------------------------------------------------------
# launch labels
# ---------------------------------------------------------------------------------------------
# labels of the primitives' own kernels; everything else a typed call launches belongs to a sort beneath it
OUTER = ("typed_", "key_encode", "key_decode", "select_", "topk_rows_", "sort_rows_", "rows_", "segments_", "search_", "runs_", "reduce_",
         "fill_")
ONE_SWEEP = ("os_hist_", "os_tables", "onesweep_")
STABLE_PAIRS = {"msd2s_prep", "msd2s_pass1_kv32", "msd2s_pass2_kv32", "msd2s_offsets"}   # (+ segment_sort_wave_e64 unless the net ran)


def inner_labels(labels):
    return {k for k in labels if not k.startswith(OUTER)}


def _is_4bit_pass(k):
    return k == "scan_table" or (k.startswith(("count_", "scatter_")) and k.endswith("_4b"))


def _is_8bit_pass(k):
    return k == "scan_table" or (k.startswith(("count_", "scatter_")) and k.endswith("_8b"))


def check_labels(config, labels, sorts, net_delta=(0, 0)):
    """Asserts that the launch labels of one typed call show the configuration reaching the inner sorts `sorts` (a list of Sort).
    net_delta: how far "stat.net_runs" and "stat.net_counting" moved over the call.  Returns the inner labels."""
    inner = inner_labels(labels)
    what = "%s: %s for %s" % (config, sorted(labels), sorts)
    assert inner, "no inner sort was launched -- " + what
    forms = [form_of(s) for s in sorts]
    if config == "default":
        # The control: every size class shows in the names.  A sort in the mid-size range may still be sent down the per-digit
        # passes by the reports of earlier sorts on the handle (adlhip.hip choose_mid_form: "only speed depends on any of this"), so
        # there the mid-size form OR the 8-bit passes; the large forms take every input and must show.
        for s, form in zip(sorts, forms):
            if form == "large":
                assert any(k.startswith("msd2") for k in inner), "no label of the large sort -- " + what
        if "mid" in forms and not any(k.startswith("mid_") for k in inner):
            assert any(_is_8bit_pass(k) and k != "scan_table" for k in inner), "neither the mid-size form nor the per-digit passes -- " + what
        bad = {k for k in inner if k.endswith("_4b") and "_soa_" not in k}   # (the (class, id) sort is on 4 bits by itself)
        assert not bad, "digits of another width: %s -- %s" % (sorted(bad), what)
    elif config == "small_partition":
        bad = {k for k in inner if k.startswith(("mid_", "msd2", "segment_sort"))}
        assert not bad, "a path with a grid barrier over 256 workgroups ran: %s -- %s" % (sorted(bad), what)
        assert tuple(net_delta) == (0, 0), "the safety net ran: %s -- %s" % (net_delta, what)
    elif config == "rank0":
        assert not any(k.startswith("mid_") for k in inner), "the mid-size form ran -- " + what
        if any(s.kind in ("keys32", "keys64", "positions") for s in sorts) and not any(s.kind == "pairs" and form_of(s) == "large" for s in sorts):
            assert not any(k.startswith("msd2") for k in inner), "whole keys took the large sort -- " + what
        if any(s.kind == "pairs" and form_of(s) == "large" for s in sorts):
            assert STABLE_PAIRS <= inner, "the stable large pair sort did not run -- " + what
    elif config == "one_sweep":
        assert any(k.startswith("os_hist_") for k in inner) and any(k.startswith("onesweep_") for k in inner), "no look-back pass -- " + what
        bad = {k for k in inner if not k.startswith(ONE_SWEEP)}
        assert not bad, "something else than the look-back passes ran: %s -- %s" % (sorted(bad), what)
    elif config == "three_kernel_4bit":
        assert any(k.startswith("count_") and k.endswith("_4b") for k in inner), "no 4-bit count -- " + what
        assert any(k.startswith("scatter_") and k.endswith("_4b") for k in inner), "no 4-bit scatter -- " + what
        bad = {k for k in inner if not _is_4bit_pass(k)}
        assert not bad, "something else than the 4-bit passes ran: %s -- %s" % (sorted(bad), what)
    else:
        raise ValueError(config)
    return inner


def check_control(labels, sorts):
    """The control of a rung, on friendly keys (uniform bits) and a handle that has sorted nothing else: no report of an earlier sort
    decides, so every inner sort above the one-workgroup limit must show the form its size class names.  If a threshold moves and a
    rung stops telling the forms apart, this fails."""
    inner = inner_labels(labels)
    what = "%s for %s" % (sorted(labels), sorts)
    forms = {form_of(s) for s in sorts if s.kind not in ("positions", "soa")}   # (the sorts that see the caller's keys)
    assert forms & {"mid", "large"}, "the rung lies in no size class above the one-workgroup sort -- " + what
    # (behind a sort of positions the mid-size form is not certain even here: that sort always overflows it, and its report may reach
    # the host before the pair sort of the same call is chosen)
    if "mid" in forms and not any(s.kind == "positions" for s in sorts):
        assert any(k.startswith("mid_") for k in inner), "no label of the mid-size form -- " + what
    if "large" in forms:
        assert any(k.startswith("msd2") for k in inner), "no label of the large sort -- " + what
    return inner


class Once:
    """expected results, computed once per key and shared by the configurations"""

    def __init__(self):
        self.have = {}
        self.computed = 0

    def get(self, key, make):
        if key not in self.have:
            self.have[key] = make()
            self.computed += 1
        return self.have[key]
