"""The inputs and the reference of tests/test_gpu_typed_shapes.py, checked on the CPU (tests/typed_shapes.py; no GPU code is involved).

The reference: expected_perm() against numpy's own order of the values where that order is the sort's (no NaN, no -0), against Python's
sorted() over tuples that spell IEEE-754 totalOrder out (sign first, then the magnitude bits) where it is not, and as a permutation whose
ties ascend in index in both orders.

The inputs: every case is there because of what the pair sort sees in one of its dwords -- a constant, two values, a few hundred, one top
byte over nearly half the keys, one value on a third of them.  The statistics are recomputed here and the property each case stands for
is asserted, so that an edit of a generator cannot quietly turn a hostile case into a friendly one.
"""
import numpy as np
import pytest

from typed_shapes import (ASC, BY_NAME, CASES, DESC, PLAIN, SPECIALS, TABLE8, TYPES, dword_stats, encoded_dwords, expected_perm,
                          ordinal_halves, shape, shapes)

N_PERM = 100_003
N_STATS = (1 << 20) + 77
ALL = [(name, case) for name in CASES for case in CASES[name]]
ALL_IDS = ["%s-%s" % nc for nc in ALL]


def total_order_key(bits, name):
    """the key of one bit pattern as a Python tuple, totalOrder spelt out: negatives first, larger magnitude first among them"""
    w = 32 if name[1:] == "32" else 64
    b = int(bits)
    if name[0] == "u":
        return (b,)
    sign, mag = b >> (w - 1), b & ((1 << (w - 1)) - 1)
    if name[0] == "i":
        return (b - (1 << w) if sign else b,)
    return (0, -mag) if sign else (1, mag)


def sorted_perm(bits, name, order):
    keys = [total_order_key(b, name) for b in bits.tolist()]
    if order == DESC:
        keys = [tuple(-c for c in k) for k in keys]
    return np.array(sorted(range(len(keys)), key=keys.__getitem__), dtype=np.int64)   # sorted() is stable


def check_is_stable_permutation(bits, perm):
    assert np.array_equal(np.sort(perm), np.arange(bits.size))
    s = bits[perm]
    tie = s[:-1] == s[1:]
    assert np.all(perm[1:][tie] > perm[:-1][tie]), "ties do not ascend in index"


@pytest.mark.parametrize("name,case", ALL, ids=ALL_IDS)
def test_expected_perm_is_a_stable_permutation_in_the_values_own_order(name, case):
    dt = BY_NAME[name][2]
    x = shape(name, case, N_PERM, 7)
    asc, desc = expected_perm(x, name, ASC), expected_perm(x, name, DESC)
    check_is_stable_permutation(x, asc)
    check_is_stable_permutation(x, desc)
    hi, lo = ordinal_halves(x[asc], name)
    assert np.all((hi[:-1] < hi[1:]) | ((hi[:-1] == hi[1:]) & (lo[:-1] <= lo[1:])))
    assert np.array_equal(x[desc][::-1], x[asc])   # the same runs, mirrored (ties apart, which the bits do not show)
    if case in PLAIN[name]:
        v = x.view(dt)
        assert not np.isnan(v.astype(np.float64)).any() and not (np.signbit(v.astype(np.float64)) & (v == 0)).any()
        assert np.array_equal(asc, np.argsort(v, kind="stable"))
        rank = np.unique(v, return_inverse=True)[1].astype(np.int64).reshape(-1)
        assert np.array_equal(desc, np.argsort(-rank, kind="stable"))
    else:
        m = 3001   # sorted() over tuples: a prefix is enough, the generators do not depend on position
        for order in (ASC, DESC):
            assert np.array_equal(expected_perm(x[:m], name, order), sorted_perm(x[:m], name, order)), order


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", [t[0] for t in TYPES])
def test_expected_perm_on_the_specials_is_total_order_spelt_out(name, order):
    sp = SPECIALS[BY_NAME[name][3]().itemsize]
    x = np.concatenate([sp, sp[::-1], sp])   # every pattern three times: ties
    perm = expected_perm(x, name, order)
    assert np.array_equal(perm, sorted_perm(x, name, order))
    check_is_stable_permutation(x, perm)
    if name[0] == "f":   # and in words: -NaN, -inf, negatives, -0, +0, positives, +inf, +NaN
        v = x[expected_perm(x, name, ASC)].view(BY_NAME[name][2])
        fin = np.flatnonzero(np.isfinite(v))
        assert np.isnan(v[:fin[0] - 3]).all() and np.signbit(v[:fin[0]]).all() and np.isneginf(v[fin[0] - 3:fin[0]]).all()
        assert np.isposinf(v[fin[-1] + 1:fin[-1] + 4]).all() and np.isnan(v[fin[-1] + 4:]).all() and not np.signbit(v[fin[-1] + 1:]).any()
        f = v[fin[0]:fin[-1] + 1]
        assert np.all(np.diff(f.astype(np.float64)) >= 0)
        z = np.flatnonzero(f == 0)
        assert z.size == 6 and np.signbit(f[z[:3]]).all() and not np.signbit(f[z[3:]]).any()


def test_shapes_are_reproducible_and_sized():
    for name in CASES:
        a, b = shapes(name, 1001, 3), shapes(name, 1001, 3)
        assert list(a) == CASES[name]
        for case in a:
            assert a[case].dtype == BY_NAME[name][3] and a[case].size == 1001 and a[case].flags.c_contiguous
            assert np.array_equal(a[case], b[case])
    assert set(TABLE8) <= set(ALL) and len(TABLE8) == 7


# what each case is there for: (dword, property); dword "lo" / "hi" of an 8-byte key, "k" the one dword of a 4-byte key
def one_value(s, n):
    return s["distinct"] == 1


def two_values(s, n):
    return s["distinct"] == 2


def at_most_256_values(s, n):
    return s["distinct"] <= 256


def many_values_with_ties(s, n):
    return 4096 < s["distinct"] < n


def heavy_top_byte(s, n):
    return s["top_byte"] >= 0.40


def heavy_value(s, n):
    return s["largest"] >= 0.25 * n


def all_distinct(s, n):
    return s["distinct"] == n


def nearly_all_distinct(s, n):   # 2^20 draws from 2^32 values collide a few hundred times
    return s["distinct"] >= 0.999 * n and s["top_byte"] < 0.02


def more_than_4096_values(s, n):
    return s["distinct"] > 4096


def repeated_value(s, n):   # +-0 and +-inf hold 10 % of the keys each (and share low dwords two by two)
    return s["largest"] >= 0.09 * n


def some_hundred_values(s, n):
    return 256 < s["distinct"] <= 4096


def every_value_three_times(s, n):
    return s["largest"] == 3 and s["distinct"] == (n + 2) // 3


INT8 = {
    "uniform_pm1000": [("hi", two_values), ("lo", some_hundred_values), ("lo", heavy_top_byte)],
    "ids": [("hi", one_value), ("lo", all_distinct)],
    "mult_2p32": [("lo", one_value), ("hi", some_hundred_values)],
    "two_specials": [("lo", two_values), ("hi", two_values)],
    "equal": [("lo", one_value), ("hi", one_value)],
    "ascending": [("lo", nearly_all_distinct), ("hi", many_values_with_ties)],
    "descending": [("lo", nearly_all_distinct), ("hi", many_values_with_ties)],
    "triples": [("hi", many_values_with_ties)],
}
GENERIC4 = {"equal": [("k", one_value)], "ascending": [("k", all_distinct)], "descending": [("k", all_distinct)],
            "triples": [("k", every_value_three_times)]}
PROPERTIES = {
    "i64": INT8,
    "u64": INT8,
    "f64": {
        "normal": [("lo", nearly_all_distinct), ("hi", many_values_with_ties), ("hi", heavy_top_byte)],
        "from_f32": [("lo", at_most_256_values), ("hi", many_values_with_ties), ("hi", heavy_top_byte)],
        "whole": [("lo", one_value), ("hi", some_hundred_values), ("hi", heavy_top_byte)],
        "nan30": [("lo", heavy_value), ("lo", many_values_with_ties), ("hi", heavy_value), ("hi", many_values_with_ties)],
        "zeros_infs": [("lo", repeated_value), ("lo", many_values_with_ties), ("hi", repeated_value), ("hi", many_values_with_ties)],
        "normal_specials": [("lo", nearly_all_distinct), ("hi", many_values_with_ties), ("hi", heavy_top_byte)],
        "two_specials": [("lo", two_values), ("hi", two_values)],
        "equal": [("lo", one_value), ("hi", one_value)],
        "ascending": [("lo", more_than_4096_values), ("hi", more_than_4096_values), ("hi", heavy_top_byte)],
        "descending": [("lo", more_than_4096_values), ("hi", more_than_4096_values), ("hi", heavy_top_byte)],
        "triples": [("lo", more_than_4096_values), ("hi", many_values_with_ties)],
    },
    "i32": dict(GENERIC4, uniform_pm1000=[("k", some_hundred_values), ("k", heavy_top_byte)], ids=[("k", all_distinct)]),
    "f32": dict(GENERIC4, normal=[("k", many_values_with_ties)],
                whole=[("k", some_hundred_values), ("k", heavy_top_byte)], nan30=[("k", heavy_value), ("k", many_values_with_ties)],
                zeros_infs=[("k", repeated_value), ("k", many_values_with_ties)]),
}


@pytest.mark.parametrize("name,case", ALL, ids=ALL_IDS)
def test_every_case_keeps_the_dword_statistics_it_is_there_for(name, case):
    x = shape(name, case, N_STATS, 7)
    lo, hi = encoded_dwords(x, name)
    stats = {"k": dword_stats(lo)} if hi is None else {"lo": dword_stats(lo), "hi": dword_stats(hi)}
    print(name, case, stats)
    props = PROPERTIES[name][case]
    assert props, "a case without a stated purpose"
    for which, prop in props:
        assert prop(stats[which], N_STATS), (name, case, which, prop.__name__, stats[which])


def test_the_table_of_the_eight_byte_dwords():
    """the seven rows the GPU tests' net outcomes are recorded for, as they were measured: n = 1 Mi + 77, ascending codec"""
    n = N_STATS
    st = {}
    for name, case in TABLE8:
        lo, hi = encoded_dwords(shape(name, case, n, 7), name)
        st[case] = dword_stats(lo), dword_stats(hi)
    lo, hi = st["uniform_pm1000"]
    assert lo["distinct"] == 2001 and 0.45 < lo["top_byte"] < 0.55 and hi["distinct"] == 2
    lo, hi = st["ids"]
    assert lo["distinct"] == n and hi["distinct"] == 1
    lo, hi = st["mult_2p32"]
    assert lo["distinct"] == 1 and hi["distinct"] == 1000
    lo, hi = st["normal"]
    assert lo["distinct"] > 0.999 * n and 900_000 < hi["distinct"] < n and 0.45 < hi["top_byte"] < 0.50
    lo, hi = st["from_f32"]
    assert lo["distinct"] == 16 and 900_000 < hi["distinct"] < n and 0.45 < hi["top_byte"] < 0.50
    lo, hi = st["whole"]
    assert lo["distinct"] == 1 and hi["distinct"] == 1000 and hi["top_byte"] > 0.99
    lo, hi = st["nan30"]
    assert 0.29 * n < lo["largest"] < 0.31 * n and lo["distinct"] > 0.69 * n and 0.29 * n < hi["largest"] < 0.31 * n


def test_encoded_dwords_order_like_the_keys():
    for name, _, _, udt in TYPES:
        sp = SPECIALS[np.dtype(udt).itemsize]
        lo, hi = encoded_dwords(sp, name)
        code = lo.astype(np.uint64) if hi is None else (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
        assert np.array_equal(np.argsort(code, kind="stable"), expected_perm(sp, name, ASC)), name
