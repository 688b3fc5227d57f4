"""Value-shaped keys for the typed sorts, and the expected order (plain numpy, no GPU; tests/test_typed_shapes.py checks this module on
the CPU, tests/test_gpu_typed_shapes.py and tests/test_gpu_typed_sort.py use it).

The typed sorts that return an order (primitives.hip typed_index_sort) run the stable {32 key bits, index} pair sort once per key dword,
and every run picks its size class and its safety nets by what ITS dword looks like.  Real int64 / float64 / float32 data gives the two
dwords of a key opposite extremes -- one all distinct and the other constant, one uniform and the other under a single top byte -- which
random bit patterns never do.  shape() makes such keys as bit patterns; dword_stats() states what each encoded dword looks like.

The expected order is stated independently of the key codec's formula: a key's ordinal is its bit pattern read as sign-magnitude (s =
the bits as a signed integer; ordinal = s if s >= 0 else -(s & MAX) - 1) for floats, the value itself for integers, and the expected
permutation is the stable argsort of the ordinal (descending: of the negated ordinal, which is exact in int64 for 4-byte keys and taken
on (high, low) halves for 8-byte keys).
"""
import numpy as np

ASC, DESC = 0, 1
# name, ADLHIP_KEY_*, the element type, its unsigned twin
TYPES = [("u32", 0, np.uint32, np.uint32), ("i32", 1, np.int32, np.uint32), ("f32", 2, np.float32, np.uint32),
         ("u64", 3, np.uint64, np.uint64), ("i64", 4, np.int64, np.uint64), ("f64", 5, np.float64, np.uint64)]
BY_NAME = {t[0]: t for t in TYPES}

# bit patterns that matter to some reading of the bits: +-0 (0x80.. is INT_MIN too), +-smallest denormal, +-smallest normal, +-largest
# finite, +-inf, quiet and signalling NaNs of both signs with distinct payloads, INT_MAX (a NaN), -1 (a NaN), 1, -2
SPECIALS = {
    4: np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff, 0x7f800000,
                 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00123, 0xffc00123, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff,
                 0xfffffffe, 0x3f800000, 0xbf800000], dtype=np.uint32),
    8: np.array([0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x0010000000000000,
                 0x8010000000000000, 0x7fefffffffffffff, 0xffefffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                 0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123, 0xfff8000000000123, 0x7ff0000000000001,
                 0xfff0000000000001, 0x7fffffffffffffff, 0xffffffffffffffff, 0xfffffffffffffffe, 0x3ff0000000000000,
                 0xbff0000000000000, 0x00000000ffffffff, 0x0000000100000000, 0xffffffff00000000], dtype=np.uint64),
}


# ---------------------------------------------------------------------------------------------
# the expected order
# ---------------------------------------------------------------------------------------------
def ordinal_halves(bits, name):
    """(high, low) int64 arrays whose lexicographic order is the order of the keys with these bit patterns."""
    w = bits.dtype.itemsize
    if name[0] == "u":
        if w == 4:
            return bits.astype(np.int64), np.zeros(bits.size, np.int64)
        return (bits >> np.uint64(32)).astype(np.int64), (bits & np.uint64(0xffffffff)).astype(np.int64)
    s = bits.view(np.int32 if w == 4 else np.int64).astype(np.int64)
    if name[0] == "f":   # sign-magnitude
        mx = np.int64(0x7fffffff if w == 4 else 0x7fffffffffffffff)
        s = np.where(s >= 0, s, -(s & mx) - 1)
    if w == 4:
        return s, np.zeros(bits.size, np.int64)
    return s >> np.int64(32), s & np.int64(0xffffffff)


def expected_perm(bits, name, order):
    hi, lo = ordinal_halves(bits, name)
    if order == DESC:
        hi, lo = -hi, -lo
    if bits.dtype.itemsize == 4:
        return np.argsort(hi, kind="stable")
    return np.lexsort((lo, hi))   # stable; the last key is the primary one


def encoded_dwords(bits, name):
    """(low, high) uint32 arrays: the dwords the ascending sort runs on, low first -- the ordinal moved into the unsigned range.  4-byte keys
    have no high dword (None).  A descending sort runs on their complements, which have the same statistics mirrored."""
    hi, lo = ordinal_halves(bits, name)
    bias = np.int64(0 if name[0] == "u" else 1 << 31)
    if bits.dtype.itemsize == 4:
        return (hi + bias).astype(np.uint32), None
    return lo.astype(np.uint32), (hi + bias).astype(np.uint32)


def dword_stats(d):
    """what a pair sort sees of a dword: how many values, how often the commonest occurs, the share of the heaviest top byte"""
    _, counts = np.unique(d, return_counts=True)
    top = np.bincount((d >> np.uint32(24)).astype(np.int64), minlength=256)
    return {"distinct": int(counts.size), "largest": int(counts.max()), "top_byte": float(top.max()) / d.size}


# ---------------------------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------------------------
IDS_BASE = 395812094 << 32   # ~1.7e18, a multiple of 2^32: ids BASE + 12345 + 1000 i share one high dword for i < 4 Mi
NAN_PATTERN = {4: 0x7fc00000, 8: 0x7ff8000000000000}   # the quiet +NaN that arithmetic produces


def _splice_specials(x, rng):
    sp = SPECIALS[x.dtype.itemsize]
    at = rng.choice(x.size, size=min(x.size // 2, 3 * sp.size), replace=False)
    x[at] = np.resize(sp, at.size)
    return x


def _ascending(name, n):
    """n strictly ascending keys in the type's own order that cross zero (signed, float) and reach into the high bits"""
    dt = BY_NAME[name][2]
    i = np.arange(n, dtype=np.int64)
    if name[0] == "f":
        return ((i - n // 2).astype(np.float64) * 0.1000000123).astype(dt)   # (steps of 0.1 stay apart in float32 too: |values| < 2^18, ulp < 0.02)
    if name == "i32":
        return ((i - n // 2) * 997).astype(dt)
    if name == "i64":
        return (i - n // 2) * np.int64(1_000_003_007)   # (odd: the low dwords are distinct; four keys or so share a high dword)
    if name == "u32":
        return (i * 2039).astype(dt)
    return np.uint64(0x7ffffff000000000) + i.astype(np.uint64) * np.uint64(1_000_003_007)   # crosses 2^63 after 69 keys


def _as_int(name, x):
    """int64 values as the type's elements; for u64 the same bits (a negative int64 is a large uint64)"""
    return x.view(np.uint64) if name == "u64" else x.astype(BY_NAME[name][2])


def _uniform_pm1000(name, n, rng):
    return _as_int(name, rng.integers(-1000, 1001, size=n))


def _ids(name, n, rng):
    i = np.arange(n, dtype=np.int64)
    if name in ("i32", "u32"):
        return (1_000_000 + 7 * i).astype(BY_NAME[name][2])
    return _as_int(name, IDS_BASE + 12345 + 1000 * i)


def _mult_2p32(name, n, rng):
    return _as_int(name, rng.integers(-500, 500, size=n) << 32)


def _normal(name, n, rng):
    return rng.standard_normal(n).astype(BY_NAME[name][2])


def _from_f32(name, n, rng):
    return rng.standard_normal(n).astype(np.float32).astype(np.float64)


def _whole(name, n, rng):
    return rng.integers(0, 1000, size=n).astype(BY_NAME[name][2])


def _nan30(name, n, rng):
    x = _normal(name, n, rng).view(BY_NAME[name][3]).copy()
    x[rng.random(n) < 0.30] = NAN_PATTERN[x.dtype.itemsize]
    return x


def _zeros_infs(name, n, rng):
    """+-0 and +-inf, 10 % each, among normals"""
    x = _normal(name, n, rng)
    pick = rng.integers(0, 10, size=n)
    for slot, v in enumerate((0.0, -0.0, np.inf, -np.inf)):
        x[pick == slot] = v
    return x


def _normal_specials(name, n, rng):
    return _splice_specials(_normal(name, n, rng).view(BY_NAME[name][3]).copy(), rng)


def _equal(name, n, rng):
    return np.full(n, {"f": 2.5, "i": -77, "u": 0xfedcba98}[name[0]], dtype=BY_NAME[name][2])


def _two_specials(name, n, rng):
    """0x00000000ffffffff and 0x0000000100000000: they differ in both dwords, in opposite directions"""
    return np.where(rng.integers(0, 2, size=n) == 1, np.uint64(0x00000000ffffffff), np.uint64(0x0000000100000000))


def _asc(name, n, rng):
    return _ascending(name, n)


def _desc(name, n, rng):
    return _ascending(name, n)[::-1]


def _triples(name, n, rng):
    return np.repeat(_ascending(name, (n + 2) // 3), 3)[:n]


_GENERIC = [("equal", _equal), ("ascending", _asc), ("descending", _desc), ("triples", _triples)]
_INT8 = [("uniform_pm1000", _uniform_pm1000), ("ids", _ids), ("mult_2p32", _mult_2p32), ("two_specials", _two_specials)]
_CASES = {
    "i64": _INT8 + _GENERIC,
    "u64": _INT8 + _GENERIC,
    "f64": [("normal", _normal), ("from_f32", _from_f32), ("whole", _whole), ("nan30", _nan30), ("zeros_infs", _zeros_infs),
            ("normal_specials", _normal_specials), ("two_specials", _two_specials)] + _GENERIC,
    "i32": [("uniform_pm1000", _uniform_pm1000), ("ids", _ids)] + _GENERIC,
    "f32": [("normal", _normal), ("whole", _whole), ("nan30", _nan30), ("zeros_infs", _zeros_infs)] + _GENERIC,
}
CASES = {name: [c for c, _ in lst] for name, lst in _CASES.items()}
# the cases whose order numpy's own comparison of the values gives as well: no NaN, no -0
PLAIN = {name: [c for c in CASES[name] if c not in ("nan30", "zeros_infs", "normal_specials")] for name in CASES}
# the seven rows of the issue's table, (type, case) by 8-byte key type
TABLE8 = [("i64", "uniform_pm1000"), ("i64", "ids"), ("i64", "mult_2p32"), ("f64", "normal"), ("f64", "from_f32"), ("f64", "whole"),
          ("f64", "nan30")]


def shape(name, case, n, seed):
    """the bit patterns (the type's unsigned twin, contiguous) of one case: n keys of type `name`"""
    fn = dict(_CASES[name])[case]
    rng = np.random.default_rng([seed, CASES[name].index(case), len(name) + ord(name[0])])
    x = np.ascontiguousarray(fn(name, n, rng))
    assert x.size == n and x.dtype in (BY_NAME[name][2], BY_NAME[name][3]), (name, case, x.dtype, x.size)
    return x.view(BY_NAME[name][3])


def shapes(name, n, seed):
    """{case name: bit patterns} for one key type"""
    return {case: shape(name, case, n, seed) for case in CASES[name]}
