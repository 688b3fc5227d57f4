"""The oracle of the set operation tests (include/adlhip.h "set operations on sorted sequences"), numpy only: take merge_oracle's stable
order of A || B, compute every element's rank inside its own input's run of its key and the lengths of that key's runs in A and in B,
and apply the keep rules of the header.  Keys and values are bit patterns in unsigned arrays throughout.
tests/test_setop_api.py checks this file against a collections.Counter multiset and against thrust's two-pointer loops."""
import numpy as np

from merge_oracle import ASC, DESC, BY_NAME, SPECIALS, TYPE_IDS, TYPES, codes, is_sorted, merge_oracle, sort_bits  # noqa: F401

INTERSECTION, UNION, DIFFERENCE, SYMMETRIC_DIFFERENCE = 0, 1, 2, 3
OPS = ("intersection", "union", "difference", "symmetric_difference")
OP_IDS = {name: i for i, name in enumerate(OPS)}


def capacity(op, na, nb):
    """the elements every output of `op` holds"""
    return na + nb if op in (UNION, SYMMETRIC_DIFFERENCE) else na


def _rank_and_count(c, other):
    """for sorted codes c: every element's rank in its run, and the length of its code's run in the sorted codes `other`"""
    first = np.searchsorted(c, c, side="left")
    rank = np.arange(c.size) - first
    count = np.searchsorted(other, c, side="right") - np.searchsorted(other, c, side="left")
    return rank, count


def keep_mask(a, b, name, op, order=ASC):
    """the keep bit of every element of a || b (a and b sorted in `order`)"""
    ca, cb = codes(a, name, order), codes(b, name, order)
    ra, n_in_b = _rank_and_count(ca, cb)
    rb, m_in_a = _rank_and_count(cb, ca)
    if op == INTERSECTION:
        ka, kb = ra < n_in_b, np.zeros(b.size, bool)
    elif op == UNION:
        ka, kb = np.ones(a.size, bool), rb >= m_in_a
    elif op == DIFFERENCE:
        ka, kb = ra >= n_in_b, np.zeros(b.size, bool)
    elif op == SYMMETRIC_DIFFERENCE:
        ka, kb = ra >= n_in_b, rb >= m_in_a
    else:
        raise ValueError("unknown op %r" % (op,))
    return np.concatenate([ka, kb])


def setop_oracle(a, b, name, op, order=ASC, va=None, vb=None):
    """(index, keys, values or None, count) of `op` on a and b (each sorted in `order`): index[j] is the position in a || b of the
    j-th result element; the result is the subsequence of the stable merge that the keep rules select"""
    index, keys, vals = merge_oracle(a, b, name, order, va, vb)
    kept = keep_mask(a, b, name, op, order)[index]
    return index[kept], keys[kept], vals[kept] if vals is not None else None, int(kept.sum())
