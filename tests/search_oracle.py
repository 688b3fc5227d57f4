"""The oracle of the sorted-search tests (include/adlhip.h "sorted search"), numpy only: encode the sequence and the needles with the
order-preserving code of the typed sorts (tests/merge_oracle.py: codes; complemented for the descending order) and take
np.searchsorted(codes(sorted), codes(needles), side).  Keys are bit patterns in unsigned arrays throughout.
tests/test_search_api.py checks this file against a plain counting loop."""
import numpy as np

from merge_oracle import ASC, BY_NAME, DESC, SPECIALS, TYPE_IDS, codes, is_sorted, sort_bits  # noqa: F401  (the tests take the tables from here)

LEFT, RIGHT = 0, 1
SIDE_NAME = {LEFT: "left", RIGHT: "right"}


def search_oracle(sorted_bits, needle_bits, name, order=ASC, side=LEFT):
    """uint32 positions: for every needle the number of elements of sorted_bits (sorted in `order`) whose code is below (RIGHT: below
    or equal to) the needle's"""
    return np.searchsorted(codes(sorted_bits, name, order), codes(needle_bits, name, order), side=SIDE_NAME[side]).astype(np.uint32)


def decode(code, name, order=ASC):
    """the bit patterns whose codes are `code`: the inverse of codes()"""
    e = ~code if order == DESC else code.copy()
    w = e.dtype.itemsize
    udt = e.dtype.type
    sign = udt(1 << (8 * w - 1))
    ones = udt((1 << (8 * w)) - 1)
    if name[0] == "i":
        e = e ^ sign
    if name[0] == "f":
        e = e ^ np.where(e & sign != 0, sign, ones).astype(udt)
    return e
