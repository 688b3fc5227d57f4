"""The oracle of the merge tests (include/adlhip.h "merge of sorted sequences"), numpy only: encode A || B with the order-preserving code
of the typed sorts (tests/compact_oracle.py: encode; complemented for the descending order), take np.argsort(codes, kind="stable") --
that is the index output -- and gather keys and values through it.  Keys and values are bit patterns in unsigned arrays throughout.
tests/test_merge_api.py checks this file against a plain two-pointer loop in which a tie takes A."""
import numpy as np

from compact_oracle import BY_NAME, SPECIALS, TYPE_IDS, TYPES, encode  # noqa: F401  (the tests take the type tables from here)

ASC, DESC = 0, 1


def codes(bits, name, order=ASC):
    """what adlhip_key_encode(key_type, order) gives for bit patterns of type `name`"""
    e = encode(bits, name)
    return ~e if order == DESC else e


def sort_bits(bits, name, order=ASC):
    """bits, stably sorted in `order`: a valid input of the merge"""
    return bits[np.argsort(codes(bits, name, order), kind="stable")]


def is_sorted(bits, name, order=ASC):
    c = codes(bits, name, order)
    return bool((c[1:] >= c[:-1]).all())


def merge_oracle(a, b, name, order=ASC, va=None, vb=None):
    """(index, keys, values or None) of the stable merge of a and b (each sorted in `order`): index[j] is the position in a || b of
    the j-th output element"""
    cat = np.concatenate([a, b])
    index = np.argsort(codes(cat, name, order), kind="stable").astype(np.uint32)
    vals = np.concatenate([va, vb])[index] if va is not None else None
    return index, cat[index], vals
