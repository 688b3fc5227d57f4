"""The oracle of the join and expansion tests (include/adlhip.h "expansion of runs and join of sorted sequences"), numpy only: the
codes of merge_oracle.py, a searchsorted of A's codes in B's for both sides, the rows per element by kind, then np.repeat.  Keys and
values are bit patterns in unsigned arrays throughout.  tests/test_join_api.py checks this file against a brute-force double loop."""
import numpy as np

from merge_oracle import ASC, DESC, BY_NAME, SPECIALS, TYPE_IDS, TYPES, codes, is_sorted, sort_bits  # noqa: F401

INNER, LEFT, SEMI, ANTI = 0, 1, 2, 3
KINDS = ("inner", "left", "semi", "anti")
KIND_IDS = {name: i for i, name in enumerate(KINDS)}
NONE = 0xFFFFFFFF


def expand_oracle(counts, values=None):
    """(run, rank, values or None, T) of the expansion of `counts`: row o belongs to the run i with start[i] <= o < start[i] + counts[i]"""
    counts = np.asarray(counts).astype(np.int64)
    total = int(counts.sum())
    start = np.cumsum(counts) - counts
    run = np.repeat(np.arange(counts.size, dtype=np.int64), counts)
    rank = np.arange(total, dtype=np.int64) - start[run]
    return run.astype(np.uint32), rank.astype(np.uint32), values[run] if values is not None else None, total


def join_counts(a, b, name, kind, order=ASC):
    """(lo, rows) per element of a: the codes of b below its code, and the rows it contributes to `kind`"""
    ca, cb = codes(a, name, order), codes(b, name, order)
    lo = np.searchsorted(cb, ca, side="left").astype(np.int64)
    m = np.searchsorted(cb, ca, side="right").astype(np.int64) - lo
    if kind == INNER:
        rows = m
    elif kind == LEFT:
        rows = np.maximum(m, 1)
    elif kind == SEMI:
        rows = np.minimum(m, 1)
    elif kind == ANTI:
        rows = (m == 0).astype(np.int64)
    else:
        raise ValueError("unknown kind %r" % (kind,))
    return lo, m, rows


def join_total(a, b, name, kind, order=ASC):
    return int(join_counts(a, b, name, kind, order)[2].sum())


def join_oracle(a, b, name, kind, order=ASC, limit=None):
    """(index_a, index_b, T) of `kind` on a and b (each sorted in `order`); with `limit`, only the first min(T, limit) rows -- computed
    without the rest, so that a count beyond 2^32 costs nothing"""
    lo, m, rows = join_counts(a, b, name, kind, order)
    total = int(rows.sum())
    if limit is not None and total > limit:
        ends = np.cumsum(rows)
        last = int(np.searchsorted(ends, limit, side="left"))        # the element that owns row limit - 1
        rows = rows[:last + 1].copy()
        rows[last] -= int(ends[last]) - limit
        lo, m = lo[:last + 1], m[:last + 1]
    run, rank, _, _ = expand_oracle(rows)
    ib = lo[run] + rank
    if kind == ANTI:
        ib[:] = NONE
    elif kind == LEFT:
        ib[m[run] == 0] = NONE
    return run, ib.astype(np.uint32), total
