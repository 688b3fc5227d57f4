"""The oracle of the stream-compaction tests (include/adlhip.h "stream compaction"), numpy only: a boolean mask -- from flag bytes, or
from encode(keys) cmp encode(threshold) with the order-preserving code of the typed sorts --, then np.flatnonzero, and a stable
concatenation for the partition.  Keys, items and values are bit patterns in unsigned arrays throughout.  tests/test_compact_api.py
checks this file against a plain Python loop."""
import numpy as np

LT, LE, GT, GE, EQ, NE = range(6)
CMPS = (LT, LE, GT, GE, EQ, NE)
CMP_NAMES = {LT: "lt", LE: "le", GT: "gt", GE: "ge", EQ: "eq", NE: "ne"}
# (name, ADLHIP_KEY_*, typed view, bit-pattern view)
TYPES = [("u32", 0, np.uint32, np.uint32), ("i32", 1, np.int32, np.uint32), ("f32", 2, np.float32, np.uint32),
         ("u64", 3, np.uint64, np.uint64), ("i64", 4, np.int64, np.uint64), ("f64", 5, np.float64, np.uint64)]
BY_NAME = {t[0]: t for t in TYPES}
TYPE_IDS = [t[0] for t in TYPES]

# +-0, denormals, the largest finite values, +-inf, quiet and signalling NaNs with payloads, the integer extremes, +-1
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


def encode(bits, name):
    """the ascending order-preserving code of bit patterns of type `name` (tests/test_gpu_reduce.py: encode)"""
    w = bits.dtype.itemsize
    udt = bits.dtype.type
    sign = udt(1 << (8 * w - 1))
    ones = udt((1 << (8 * w)) - 1)
    e = bits.copy()
    if name[0] == "i":
        e ^= sign
    if name[0] == "f":
        e ^= np.where(bits & sign != 0, ones, sign).astype(udt)
    return e


def mask_from_flags(flags):
    return np.asarray(flags).view(np.uint8) != 0


def mask_from_cmp(kbits, name, cmp, threshold_bits):
    """kbits[i] cmp threshold in the ascending order of the typed sorts; threshold_bits: one bit pattern of kbits' dtype"""
    e = encode(kbits, name)
    t = encode(np.array([threshold_bits], dtype=kbits.dtype), name)[0]
    return {LT: e < t, LE: e <= t, GT: e > t, GE: e >= t, EQ: e == t, NE: e != t}[cmp]


def compact_oracle(mask, partition, arrays):
    """(S, index, outputs): the positions of the selected elements in input order -- followed by those of the rejected ones with
    `partition` --, and arrays[k] gathered through them"""
    mask = np.asarray(mask, dtype=bool)
    sel = np.flatnonzero(mask)
    order = np.concatenate([sel, np.flatnonzero(~mask)]) if partition else sel
    return sel.size, order.astype(np.uint32), [a[order] for a in arrays]
