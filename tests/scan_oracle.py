"""The numpy oracle of the typed scans (include/adlhip.h "typed scans"), shared by tests/test_scan_api.py, which checks it against a
plain Python loop, and tests/test_gpu_scan.py, which checks the device against it.  Everything is bit patterns: values travel as
unsigned integers of their width.

    segment ids     from the key bits: a head is position 0 or a position whose key differs from the one in front (None: one segment)
    integer sums    np.cumsum on the unsigned view (it wraps) minus the prefix carried into the segment
    float sums      ONLY for values that are integers stored as floats, whose partial sums stay below 2^53: the same cumsum in float64,
                    which is then exact, so the result is the one of every association
    min / max       np.maximum.accumulate on (segment id << 32 | rank of the order-preserving code), min on the complemented code
    exclusive       init (or the operator's identity pattern) at heads, inc[i - 1] or op(init, inc[i - 1]) elsewhere
"""
import struct

import numpy as np

SUM, MIN, MAX = 0, 1, 2
OPS = {"sum": SUM, "min": MIN, "max": MAX}
# name -> (ADLHIP_KEY_* code, numpy type, unsigned type of the same width)
TYPES = {"u32": (0, np.uint32, np.uint32), "i32": (1, np.int32, np.uint32), "f32": (2, np.float32, np.uint32),
         "u64": (3, np.uint64, np.uint64), "i64": (4, np.int64, np.uint64), "f64": (5, np.float64, np.uint64)}

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
    """the order-preserving code of include/adlhip.h "typed keys", ascending"""
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


def decode(code, name):
    w = code.dtype.itemsize
    udt = code.dtype.type
    sign = udt(1 << (8 * w - 1))
    if name[0] == "i":
        return code ^ sign
    if name[0] == "f":
        return np.where(code & sign != 0, code ^ sign, ~code).astype(udt)
    return code.copy()


def identity_bits(vname, op):
    """what an exclusive scan without an init writes at a head: zero bits; the decode of the all-ones code (MIN), of code 0 (MAX)"""
    udt = TYPES[vname][2]
    if op == SUM:
        return udt(0)
    code = np.array([(1 << (8 * np.dtype(udt).itemsize)) - 1 if op == MIN else 0], dtype=udt)
    return decode(code, vname)[0]


def heads_of(kbits, n):
    if kbits is None:
        h = np.zeros(n, dtype=bool)
        h[:1] = True
        return h
    assert kbits.size == n
    return np.concatenate([[True], kbits[1:] != kbits[:-1]])[:n]


def combine(a_bits, b_bits, vname, op):
    """op(a, b) element-wise on bit patterns, a the left operand"""
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    a_bits = np.asarray(a_bits, dtype=udt)
    b_bits = np.asarray(b_bits, dtype=udt)
    if op == SUM and vname[0] == "f":
        with np.errstate(all="ignore"):
            return (a_bits.view(dt) + b_bits.view(dt)).astype(dt).view(udt)
    if op == SUM:
        return (a_bits + b_bits).astype(udt)
    ca, cb = encode(a_bits, vname), encode(b_bits, vname)
    return decode(np.minimum(ca, cb) if op == MIN else np.maximum(ca, cb), vname)


def inclusive_oracle(kbits, vbits, vname, op):
    n = vbits.size
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    assert vbits.dtype == udt
    if n == 0:
        return vbits.copy()
    heads = heads_of(kbits, n)
    seg = np.cumsum(heads) - 1                       # segment id of every element
    start = np.flatnonzero(heads)[seg]               # where its segment starts
    if op == SUM and vname[0] == "f":
        with np.errstate(all="ignore"):
            x = vbits.view(dt).astype(np.float64)
        x[np.bincount(seg)[seg] == 1] = 0.0          # a segment of one element is any bits: it comes back as it is (below)
        assert np.array_equal(x, np.rint(x)) and np.abs(x).sum() < 2.0 ** 53, "the float-sum oracle is for integers stored as floats"
        c = np.cumsum(x)
        inc = (c - (c[start] - x[start])).astype(dt).view(udt)
    elif op == SUM:
        c = np.cumsum(vbits, dtype=udt)
        inc = (c - (c[start] - vbits[start])).astype(udt)
    else:
        code = encode(vbits, vname)
        if op == MIN:
            code = ~code
        uniq, rank = np.unique(code, return_inverse=True)
        folded = (seg.astype(np.uint64) << np.uint64(32)) | rank.astype(np.uint64)
        best = uniq[(np.maximum.accumulate(folded) & np.uint64(0xffffffff)).astype(np.int64)]
        inc = decode(~best if op == MIN else best, vname)
    inc = inc.astype(udt)
    inc[heads] = vbits[heads]                        # a segment's first element, bit for bit (the float cast would quiet a NaN)
    return inc


def exclusive_from_inclusive(inc, heads, vname, op, init_bits=None):
    """the contract: init (or the identity pattern) at heads; elsewhere inc[i - 1], or op(init, inc[i - 1]) with an init"""
    udt = TYPES[vname][2]
    out = np.empty_like(inc)
    if inc.size == 0:
        return out
    prev = np.concatenate([inc[:1], inc[:-1]])
    out[:] = prev if init_bits is None else combine(np.full(inc.size, init_bits, dtype=udt), prev, vname, op)
    out[heads] = identity_bits(vname, op) if init_bits is None else udt(init_bits)
    return out


def scan_oracle(kbits, vbits, vname, op, exclusive=False, init_bits=None):
    inc = inclusive_oracle(kbits, vbits, vname, op)
    if not exclusive:
        assert init_bits is None
        return inc
    return exclusive_from_inclusive(inc, heads_of(kbits, vbits.size), vname, op, init_bits)


# ---------------------------------------------------------------------------------------------
# the same, element by element in plain Python (what test_scan_api.py holds the oracle against)
# ---------------------------------------------------------------------------------------------
def _total_order_key(bits, name):
    """where a value stands in the ascending order of the typed sorts, stated without the codec: integers by value; floats by sign, then
    magnitude bits (IEEE-754 totalOrder)"""
    w = 4 if name.endswith("32") else 8
    if name[0] == "u":
        return bits
    signed = bits - (1 << (8 * w)) if bits >> (8 * w - 1) else bits
    if name[0] == "i":
        return signed
    mag = bits & ((1 << (8 * w - 1)) - 1)
    return -mag - 1 if bits >> (8 * w - 1) else mag


def _loop_op(a, b, vname, op):
    w = 4 if vname.endswith("32") else 8
    if op == SUM and vname[0] == "f":
        fi, ff = ("<I", "<f") if w == 4 else ("<Q", "<d")
        x = struct.unpack(ff, struct.pack(fi, a))[0]
        y = struct.unpack(ff, struct.pack(fi, b))[0]
        s = np.float32(x) + np.float32(y) if w == 4 else x + y
        return struct.unpack(fi, struct.pack(ff, float(s)))[0]
    if op == SUM:
        return (a + b) & ((1 << (8 * w)) - 1)
    ka, kb = _total_order_key(a, vname), _total_order_key(b, vname)
    if op == MIN:
        return b if kb < ka else a
    return b if kb > ka else a


def _loop_identity(vname, op):
    w = 4 if vname.endswith("32") else 8
    if op == SUM:
        return 0
    every = {"u": (0, (1 << (8 * w)) - 1), "i": (1 << (8 * w - 1), (1 << (8 * w - 1)) - 1), "f": ((1 << (8 * w)) - 1, (1 << (8 * w - 1)) - 1)}
    lo, hi = every[vname[0]]          # the first / last pattern in ascending order
    return hi if op == MIN else lo


def loop_scan(kbits, vbits, vname, op, exclusive=False, init_bits=None):
    keys = kbits.tolist() if kbits is not None else None
    out, acc = [], None
    for i, v in enumerate(vbits.tolist()):
        head = i == 0 or (keys is not None and keys[i] != keys[i - 1])
        if exclusive:
            if head:
                out.append(_loop_identity(vname, op) if init_bits is None else int(init_bits))
            else:
                out.append(acc if init_bits is None else _loop_op(int(init_bits), acc, vname, op))
        acc = v if head else _loop_op(acc, v, vname, op)
        if not exclusive:
            out.append(acc)
    return np.array(out, dtype=vbits.dtype)
