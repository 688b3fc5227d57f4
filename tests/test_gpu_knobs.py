"""Every knob of adlhip_set_param / adlhip_get_param: what it accepts, what it normalises, what it refuses and in which words.

The tables below are literal: ranges and refusal texts as the C ABI has always given them.  One handle serves every test of the knobs;
the environment switches that set six defaults at handle creation are read by two child processes, one handle each.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oclradixsort_amd import AdlHipError, Buffer, DeviceUtils, Pprims

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INT_MAX = 2**31 - 1

# name: (lowest, highest, refusal)
PLAIN = {
    "sort.algo": (-1, 1, "sort.algo must be -1, 0 or 1"),
    "sort.mid": (0, 3, "sort.mid must be 0 (off), 1 (on), 2 (keys: always the two-launch form) or 3 (always the three-launch form)"),
    "sort.msd2": (0, 5, "sort.msd2 must be 0 (off), 1 (on), 2 (always, from 1 Mi elements; forms by size), 3 (always the stable passes), "
                        "4 (always the cursor passes for whole keys) or 5 (always the hybrid form for whole keys)"),
    "sort.persist": (0, 1, "sort.persist must be 0 (one tile per workgroup, round 3) or 1 (persistent prefetching passes + 16-bit finish)"),
    "sort.dict": (0, 1, "sort.dict must be 0 (off) or 1 (counting sort for keys that take few distinct values)"),
    "sort.binfinish": (0, 2, "sort.binfinish must be 0 (LSD finish), 1 (binning finish for whole u64 keys from 24 Mi keys up) or 2 (always, u32 keys too)"),
    "topk.algo": (-1, 1, "topk.algo must be -1 (by k), 0 (always the full argsort) or 1 (always the selection)"),
    "topk.rows_algo": (-1, 1, "topk.rows_algo must be -1 (by k and cols), 0 (always the per-row loop) or 1 (always the row kernel)"),
    "debug.topk_rows_grid": (0, None, "debug.topk_rows_grid must be >= 0"),
    "debug.unique_grid": (0, None, "debug.unique_grid must be >= 0"),
    "debug.reduce_grid": (0, None, "debug.reduce_grid must be >= 0"),
    "debug.scan_grid": (0, None, "debug.scan_grid must be >= 0"),
    "debug.compact_grid": (0, None, "debug.compact_grid must be >= 0"),
    "debug.histogram_grid": (0, None, "debug.histogram_grid must be >= 0"),
    "debug.persist_grid": (0, 4096, "debug.persist_grid must be in [0, 4096]"),
}
# name: ({value set: value read back}, [refused values], refusal).  "R" stands for the device's resident workgroup count
SPECIAL = {
    "sort.digit_bits": ({4: 4, 8: 8}, [3, 5, 6, 7, 9, 0, -1], "sort.digit_bits must be 4 or 8"),
    "unique.algo": ({1: 1, -1: -1}, [-2, 0, 2], "unique.algo must be -1 (by the outputs asked) or 1 (always the index path)"),
    "sort.tile": ({-1: -1, 0: 0, 3: 3}, [-2, 4, 6], "sort.tile must be in [-1,4)"),
    "sort.net_lookback": ({0: 0, 1: 1, 5: 1, -3: 1, INT_MAX: 1}, [], None),
    "partition.lookback": ({0: 0, 1: 1, 5: 1, -3: 1, INT_MAX: 1}, [], None),
    "profile": ({1: 1, 0: 0, 5: 1, -3: 1}, [], None),
    "debug.histogram_lds_bins": ({1: 1, 8192: 8192, 100: 100, 0: 8192}, [-1, 8193], "debug.histogram_lds_bins must be in [1, 8192], or 0 for the default"),
    "debug.resident_wgs": ({1: 1, INT_MAX: INT_MAX, 0: "R"}, [-1], "debug.resident_wgs must be >= 0"),
    "sort.rank": ({0: 0}, [-1, 2], "sort.rank must be 0 or 1"),   # (the value 1: test_sort_rank_one_needs_the_self_test)
}
GET_ONLY = ["stat.net_runs", "stat.net_counting", "debug.idle_dirty", "debug.idle_first", "sort.lds_ordered"] + ["debug.net_stamp%d" % i for i in range(10)]
READABLE = list(PLAIN) + list(SPECIAL)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    before = {k: d.getParam(k) for k in READABLE}
    yield d
    try:
        assert {k: d.getParam(k) for k in READABLE} == before, "a test left a knob changed"
    finally:
        DeviceUtils.deallocate(d)


def refused(dev, name, value, text):
    before = dev.getParam(name)
    with pytest.raises(AdlHipError) as e:
        dev.setParam(name, value)
    assert str(e.value) == "adlhip_set_param failed: " + text, (name, value)
    assert dev.getParam(name) == before, (name, value)


def set_and_check_alone(dev, name, value, want):
    """set, read back, and no other knob has moved"""
    others = {k: dev.getParam(k) for k in READABLE if k != name}
    dev.setParam(name, value)
    assert dev.getParam(name) == want, (name, value)
    assert {k: dev.getParam(k) for k in others} == others, (name, value)


def test_fresh_handle_is_idle(dev):
    assert dev.getParam("debug.idle_dirty") == 0
    assert dev.getParam("debug.idle_first") == 0


@pytest.mark.parametrize("name", list(PLAIN))
def test_plain_knob_round_trips_and_refuses(dev, name):
    lo, hi, text = PLAIN[name]
    first = dev.getParam(name)
    try:
        for v in (lo, hi if hi is not None else INT_MAX, lo):
            set_and_check_alone(dev, name, v, v)
        refused(dev, name, lo - 1, text)
        if hi is not None:
            refused(dev, name, hi + 1, text)
        refused(dev, name, -INT_MAX - 1, text)
    finally:
        dev.setParam(name, first)


@pytest.mark.parametrize("name", list(SPECIAL))
def test_knob_with_a_rule_of_its_own(dev, name):
    accepted, bad, text = SPECIAL[name]
    resident = dev.getParam("debug.resident_wgs")
    assert resident > 0
    first = dev.getParam(name)
    try:
        for v, want in accepted.items():
            set_and_check_alone(dev, name, v, resident if want == "R" else want)
        for v in bad:
            refused(dev, name, v, text)
    finally:
        dev.setParam(name, 0 if name == "debug.resident_wgs" else first)


def test_sort_rank_one_needs_the_self_test(dev):
    first = dev.getParam("sort.rank")
    ordered = dev.getParam("sort.lds_ordered")
    assert ordered in (0, 1) and first == ordered
    dev.setParam("sort.rank", 0)
    if ordered:
        set_and_check_alone(dev, "sort.rank", 1, 1)
    else:
        refused(dev, "sort.rank", 1, "sort.rank = 1 needs lane-ordered DS atomics; the device self-test failed")
    dev.setParam("sort.rank", first)


@pytest.mark.parametrize("name", GET_ONLY)
def test_get_only_names_cannot_be_set(dev, name):
    before = dev.getParam(name)
    with pytest.raises(AdlHipError) as e:
        dev.setParam(name, 0)
    assert str(e.value) == "adlhip_set_param failed: unknown parameter '%s'" % name
    assert dev.getParam(name) == before


@pytest.mark.parametrize("name", ["debug.idle_poke", "sort.no_such_knob", "", "sort.alg", "sort.algo ", "debug.net_stamp10", "debug.net_stamp"])
def test_names_that_cannot_be_read(dev, name):
    with pytest.raises(AdlHipError) as e:
        dev.getParam(name)
    assert str(e.value) == "adlhip_get_param failed: unknown parameter '%s'" % name


def test_invented_name_cannot_be_set(dev):
    with pytest.raises(AdlHipError) as e:
        dev.setParam("sort.no_such_knob", 1)
    assert str(e.value) == "adlhip_set_param failed: unknown parameter 'sort.no_such_knob'"


def test_idle_poke_refuses_a_word_outside_its_regions(dev):
    text = "debug.idle_poke: no word %u in region %d (region << 24 | word; regions 1 d_msd2, 2 d_mid_hist, 3 d_dict, 4 d_fault)"
    for region, word in ((0, 5), (5, 0), (4, 16), (1, 8192 + 65536 + 64)):
        with pytest.raises(AdlHipError) as e:
            dev.setParam("debug.idle_poke", region << 24 | word)
        assert str(e.value) == "adlhip_set_param failed: " + text % (word, region)
    assert dev.getParam("debug.idle_dirty") == 0


def test_sort_after_the_round_trips(dev):
    """(runs last in this file: every knob has been set and put back)"""
    n = 20000
    keys = oracle.keys_u32(n, seed=2024)
    p = Pprims()
    buf = Buffer(dev, n, np.uint32)
    try:
        buf.write(keys)
        p.radixSort(dev, buf, n)
        assert np.array_equal(buf.toHost(), np.sort(keys))
    finally:
        buf.release()
        p.close()
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# the six defaults a handle takes from the environment at creation
# ---------------------------------------------------------------------------------------------
ENV_KNOBS = {"ADLHIP_SORT_ALGO": "sort.algo", "ADLHIP_SORT_TILE": "sort.tile", "ADLHIP_SORT_RANK": "sort.rank", "ADLHIP_SORT_MID": "sort.mid",
             "ADLHIP_SORT_MSD2": "sort.msd2", "ADLHIP_DIGIT_BITS": "sort.digit_bits"}
CHILD = """
import json, sys
sys.path.insert(0, %r)
from oclradixsort_amd import DeviceUtils
d = DeviceUtils.allocate()
print(json.dumps({k: d.getParam(k) for k in %r}))
DeviceUtils.deallocate(d)
"""


def knobs_of_a_fresh_process(env):
    names = sorted(ENV_KNOBS.values()) + ["sort.lds_ordered"]
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, names)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_environment_switches():
    """One child after the other.  Valid values are taken; out of range, each switch clamps its own way: the tile, the algorithm and the
    large sort keep their defaults (ADLHIP_SORT_MSD2 takes 0..2 only), ADLHIP_SORT_MID and ADLHIP_SORT_RANK are read as flags (the rank
    ANDed with the self-test's result), and a digit width other than 4 means 8.  A tile index and a digit width that
    earlier versions took (6, 7) are out of range like any other."""
    got = knobs_of_a_fresh_process({"ADLHIP_SORT_ALGO": "1", "ADLHIP_SORT_TILE": "3", "ADLHIP_SORT_RANK": "0", "ADLHIP_SORT_MID": "0",
                                    "ADLHIP_SORT_MSD2": "2", "ADLHIP_DIGIT_BITS": "4"})
    ordered = got.pop("sort.lds_ordered")
    assert got == {"sort.algo": 1, "sort.tile": 3, "sort.rank": 0, "sort.mid": 0, "sort.msd2": 2, "sort.digit_bits": 4}
    got = knobs_of_a_fresh_process({"ADLHIP_SORT_ALGO": "2", "ADLHIP_SORT_TILE": "99", "ADLHIP_SORT_RANK": "7", "ADLHIP_SORT_MID": "5",
                                    "ADLHIP_SORT_MSD2": "3", "ADLHIP_DIGIT_BITS": "5"})
    assert got.pop("sort.lds_ordered") == ordered
    assert got == {"sort.algo": -1, "sort.tile": -1, "sort.rank": ordered, "sort.mid": 1, "sort.msd2": 1, "sort.digit_bits": 8}
    got = knobs_of_a_fresh_process({"ADLHIP_SORT_TILE": "6", "ADLHIP_DIGIT_BITS": "7"})
    assert got.pop("sort.lds_ordered") == ordered
    assert got == {"sort.algo": -1, "sort.tile": -1, "sort.rank": ordered, "sort.mid": 1, "sort.msd2": 1, "sort.digit_bits": 8}
