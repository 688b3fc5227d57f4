"""The oracle of the histogram tests (include/adlhip.h "histograms"), numpy only, on key codes: the order-preserving code of the typed
sorts (tests/compact_oracle.py: encode) of keys and edges, bin = searchsorted(edge codes, code, "right") - 1 where that lies in
[0, num_bins), plus the rule of the closed last bin; np.bincount of the values in range for the bincount.  Keys and edges are bit
patterns in unsigned arrays throughout.  tests/test_histogram_api.py checks this file against a plain Python loop and against
numpy.histogram."""
import numpy as np

from compact_oracle import BY_NAME, SPECIALS, TYPE_IDS, TYPES, encode  # noqa: F401  (the tests take the type tables from here)

INT_IDS = [n for n in TYPE_IDS if n[0] != "f"]

# the special keys by type: +-0, +-inf, +-NaN with payloads, denormals (floats); the integer extremes, 0, +-1 (integers) -- as bits
SPECIAL_KEYS = {
    "f32": SPECIALS[4], "f64": SPECIALS[8],
    "u32": np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff], dtype=np.uint32),
    "i32": np.array([0, 1, 0xffffffff, 0x7fffffff, 0x80000000, 0x80000001, 0x7ffffffe], dtype=np.uint32),
    "u64": np.array([0, 1, 0xffffffff, 0x100000000, 0x7fffffffffffffff, 0x8000000000000000, 0xffffffffffffffff], dtype=np.uint64),
    "i64": np.array([0, 1, 0xffffffffffffffff, 0xffffffff, 0x100000000, 0x7fffffffffffffff, 0x8000000000000000, 0xffffffff00000000],
                    dtype=np.uint64),
}


def sort_edges(ebits, name):
    """the bit patterns in the ascending order of the typed sorts"""
    return ebits[np.argsort(encode(ebits, name), kind="stable")]


def histogram_range_oracle(kbits, name, ebits, include_upper):
    """uint32 counts of the ebits.size - 1 bins: bin b takes the keys with edge[b] <= key < edge[b + 1] on codes; with include_upper a
    key whose bits equal the last edge's goes to the last bin whose lower edge is below the last edge (the last bin if there is none)"""
    kc, ec = encode(kbits, name), encode(ebits, name)
    bins = ebits.size - 1
    b = np.searchsorted(ec, kc, side="right").astype(np.int64) - 1
    valid = (b >= 0) & (b < bins)
    counts = np.bincount(b[valid], minlength=bins).astype(np.uint32)
    if include_upper:
        below = np.flatnonzero(ec[:bins] < ec[bins])
        upper_bin = int(below[-1]) if below.size else bins - 1
        counts[upper_bin] += np.uint32(np.count_nonzero(kc == ec[bins]))
    return counts


def bincount_oracle(kbits, name, num_bins):
    """uint32 counts of the values 0 .. num_bins - 1 among keys of the integer type `name`"""
    assert name[0] != "f"
    v = kbits.view(BY_NAME[name][2])
    if name[0] == "i":
        ok = (v >= 0) & (v < num_bins)
    else:
        ok = v < np.uint64(num_bins)
    return np.bincount(v[ok].astype(np.int64), minlength=num_bins).astype(np.uint32)
