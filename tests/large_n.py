"""Inputs whose results have a closed form, and the verifier that compares a result with its form chunk by chunk (plain torch, any
device; tests/test_large_n_forms.py checks every form against numpy on the CPU, tests/test_gpu_large_n.py uses them past 2^31
elements, where neither a host reference nor a read-back is affordable).

A FORM is a function of an int64 tensor of indices that returns an int64 tensor of the same shape: the input element i, or the expected
output element j.  Forms take arbitrary index tensors, not ranges, so that `keys_in[index[j]]` is the input form applied to the index
tensor and needs no gather from memory.  All arithmetic is int64 and stays below 2^63; fill() and the check_* functions walk their
arrays in chunks of CHUNK elements (at most 2^28), so that no temporary is larger than that.

Bit patterns.  4-byte elements live in int32 tensors, 8-byte elements in int64 tensors; a form speaks of 4-byte elements as the
unsigned reading 0 .. 2^32 - 1 of their bits (read back as int32.to(int64) & 0xffffffff), of 8-byte elements as the int64 with the same
bits.

Key types.  ordinal_to_bits() maps an ordinal -- the rank of a key among ALL keys of its type -- to the key's bits, by a monotone
bijection stated independently of the codec (as typed_shapes.ordinal_halves states the inverse): the value itself for unsigned keys,
the ordinal minus the midpoint for signed keys, the sign-magnitude reading for floats, so that NaN patterns and -0 occur and order by
totalOrder.

Why two elementwise properties pin the index of a sort with duplicate keys (check_gather, check_rising):
  1. keys_out is compared exactly, so for every key v the slots j with keys_out[j] == v are one stretch, as long as v occurs in the input;
  2. check_gather: keys_in[index[j]] == keys_out[j], so every slot of that stretch holds a position of v in the input;
  3. check_rising: inside the stretch the positions rise strictly, so they are distinct; count(v) distinct positions of v are ALL
     positions of v, in ascending order -- the stable permutation and no other.
"""
import torch

CHUNK = 1 << 24          # elements per step of fill() and the checks; tests on a GPU raise it to 2^28
M32 = 0xffffffff
S32 = 0x80000000
MIN64 = -(1 << 63)
PRIME_A = 1_000_000_007  # the multiplier of Perm: a prime below 2^31
TRI7 = (1, 3, 6, 10, 15, 21, 28)

ASC, DESC = 0, 1
KEY_TYPES = {"u32": 0, "i32": 1, "f32": 2, "u64": 3, "i64": 4, "f64": 5}   # ADLHIP_KEY_*


class Mismatch(AssertionError):
    """what a check raises; .index is the global index of the first element that is wrong"""

    def __init__(self, what, index, got, want, note=""):
        self.index, self.got, self.want = int(index), got, want
        AssertionError.__init__(self, "%s: first mismatch at %d: got %s, wanted %s%s" % (what, self.index, got, want, note))


def chunks(n, step=None):
    step = step or CHUNK
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def arange(lo, hi, device):
    return torch.arange(lo, hi, dtype=torch.int64, device=device)


def to_i32(v):
    """the int32 tensor with the low 32 bits of the int64 values"""
    return (((v & M32) ^ S32) - S32).to(torch.int32)


def from_u32(t):
    return t.to(torch.int64) & M32


def as_pattern(t):
    """a result tensor as the int64 values the forms speak in"""
    if t.dtype == torch.int64:
        return t
    if t.dtype == torch.int32:
        return from_u32(t)
    return t.to(torch.int64)   # uint8 flags


def fill(out, form, n=None, base=0):
    """out[base + i] = form(i) for i < n, chunk by chunk, on out's device; returns out"""
    n = out.numel() - base if n is None else n
    for lo, hi in chunks(n):
        v = form(arange(lo, hi, out.device))
        out[base + lo:base + hi] = to_i32(v) if out.dtype == torch.int32 else v.to(out.dtype)
    return out


def _want_pattern(v, dtype):
    return v & M32 if dtype == torch.int32 else v


def check_equal(got, want_fn, n, what):
    """got[j] == want_fn(j) for every j < n, as bit patterns; raises Mismatch for the first j that differs"""
    assert got.numel() >= n, (what, got.numel(), n)
    for lo, hi in chunks(n):
        g = as_pattern(got[lo:hi])
        w = _want_pattern(want_fn(arange(lo, hi, got.device)), got.dtype)
        ne = g != w
        if bool(ne.any()):
            k = int(ne.nonzero()[0, 0])
            raise Mismatch(what, lo + k, int(g[k]), int(w[k]))


def checksum(t, n):
    """a position-dependent 63-bit checksum of the first n elements (wrap-around int64 arithmetic); a python int"""
    acc = 0
    for lo, hi in chunks(n):
        i = arange(lo, hi, t.device)
        acc = (acc + int(((as_pattern(t[lo:hi]) ^ (i * 0x9e3779b1)) * (2 * i + 1)).sum())) & ((1 << 63) - 1)
    return acc


def form_checksum(form, n, device, dtype):
    """the checksum a tensor of `dtype` filled with the form would have"""
    acc = 0
    for lo, hi in chunks(n):
        i = arange(lo, hi, device)
        acc = (acc + int(((_want_pattern(form(i), dtype) ^ (i * 0x9e3779b1)) * (2 * i + 1)).sum())) & ((1 << 63) - 1)
    return acc


def check_count(got, want, what):
    """a count word (a tensor of one u32) against the closed-form count"""
    g = int(from_u32(got.reshape(-1)[:1])[0])
    if g != int(want):
        raise Mismatch(what, 0, g, int(want), " (a count)")


def check_range(index, n_out, bound, what, conv=from_u32):
    """0 <= index[j] < bound for j < n_out; conv: a chunk of `index` as int64 positions (u32 indices by default, or the value half of
    a key-value pair)"""
    for lo, hi in chunks(n_out):
        ix = conv(index[lo:hi])
        bad = ix >= bound
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise Mismatch(what + " (index range)", lo + k, int(ix[k]), "< %d" % bound)


def check_gather(index, in_form, out_form, n_out, n_in, what, conv=from_u32):
    """keys_in[index[j]] == keys_out[j] for j < n_out, with keys_in and keys_out given by their forms"""
    check_range(index, n_out, n_in, what, conv)
    for lo, hi in chunks(n_out):
        ix = conv(index[lo:hi])
        g = in_form(ix)
        w = out_form(arange(lo, hi, index.device))
        ne = g != w
        if bool(ne.any()):
            k = int(ne.nonzero()[0, 0])
            raise Mismatch(what + " (key at index)", lo + k, "index %d with key %d" % (int(ix[k]), int(g[k])), "a key %d" % int(w[k]))


def check_rising(index, out_form, n_out, what, everywhere=False, conv=from_u32):
    """index[j] < index[j + 1] wherever keys_out[j] == keys_out[j + 1] (everywhere: for every j); Mismatch.index is j + 1"""
    for lo, hi in chunks(n_out):
        hi1 = min(hi + 1, n_out)   # one element of overlap: the pair that straddles two chunks
        if hi1 - lo < 2:
            continue
        ix = conv(index[lo:hi1])
        bad = ix[1:] <= ix[:-1]
        if not everywhere:
            w = out_form(arange(lo, hi1, index.device))
            bad &= w[1:] == w[:-1]
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise Mismatch(what + " (indices rise)", lo + k + 1, int(ix[k + 1]), "> %d" % int(ix[k]))


# ---------------------------------------------------------------------------------------------------------------------
# the permutation
# ---------------------------------------------------------------------------------------------------------------------
class Perm:
    """P(i) = (i A + B) mod n, a permutation of 0 .. n - 1 (A is prime and does not divide n, so gcd(A, n) = 1), and its inverse
    inv(j) = ((j - B) A^-1) mod n.  n < 2^32 and A < 2^31 keep i A + B below 2^63; the inverse multiplies in two 16-bit halves."""

    def __init__(self, n, a=PRIME_A, b=12345):
        assert 0 < n < (1 << 32) and a < (1 << 31) and n % a != 0 and 0 <= b < (1 << 20)
        self.n, self.a, self.b = n, a, b
        self.ainv = pow(a % n, -1, n) if n > 1 else 0

    def __call__(self, i):
        return (i * self.a + self.b) % self.n

    def inv(self, j):
        x = (j - self.b) % self.n
        hi, lo = self.ainv >> 16, self.ainv & 0xffff
        return ((((x * hi) % self.n) << 16) + x * lo) % self.n


# ---------------------------------------------------------------------------------------------------------------------
# key types
# ---------------------------------------------------------------------------------------------------------------------
def ordinal_to_bits(o, ktype):
    """the bits of the key of type ktype with ordinal o.  4-byte types: 0 <= o < 2^32, the result is the unsigned reading of the bits.
    8-byte types: o is SIGNED, -2^63 <= o < 2^63 (the rank minus 2^63), the result the int64 with the key's bits."""
    if ktype in ("u32", "i32", "f32"):
        if ktype == "u32":
            return o
        s = o - S32                                   # the signed value (i32) / the sign-magnitude reading (f32)
        if ktype == "i32":
            return s & M32
        return torch.where(s >= 0, s, (~s) | S32) & M32   # s < 0: sign bit set, magnitude -s - 1
    if ktype == "u64":
        return o ^ MIN64
    if ktype == "i64":
        return o
    return torch.where(o >= 0, o, (~o) | MIN64)


def key_bytes(ktype):
    return 4 if ktype.endswith("32") else 8


class SortForm:
    """n keys of one type whose sort has a closed form: ordinals r(i) = P(i) >> shift, mapped to the type.  4-byte keys: ordinal
    base + r with base chosen so that the keys straddle the midpoint (negative and positive values, both float signs, NaNs only when
    asked by base).  8-byte keys: ordinal r C + D with C = 2^33 + 12345, so that both dwords vary, D = -2^61: n C + D < 2^63 for
    n < 2^29.9.  shift == 0: the argsort is P's inverse; shift > 0: ties, the index is pinned by check_gather and check_rising."""

    C8 = (1 << 33) + 12345
    D8 = -(1 << 61)

    def __init__(self, n, ktype, order=ASC, shift=0, base=None):
        self.n, self.ktype, self.order, self.shift, self.p = n, ktype, order, shift, Perm(n)
        self.wide = key_bytes(ktype) == 8
        if self.wide:
            assert n * self.C8 + self.D8 < (1 << 63)
        else:
            self.base = (S32 - n // 2) if base is None else base
            assert 0 <= self.base and self.base + n <= (1 << 32)

    def _key(self, r):
        o = r * self.C8 + self.D8 if self.wide else self.base + r
        return ordinal_to_bits(o, self.ktype)

    def rank_in(self, i):
        return self.p(i) >> self.shift

    def rank_out(self, j):
        return (j if self.order == ASC else self.n - 1 - j) >> self.shift

    def keys_in(self, i):
        return self._key(self.rank_in(i))

    def keys_out(self, j):
        return self._key(self.rank_out(j))

    def index_out(self, j):
        assert self.shift == 0
        return self.p.inv(j if self.order == ASC else self.n - 1 - j)

    def values_in(self, i):
        """a value that names its element: the position, with the high bits set too for 8-byte values"""
        return i * 0x100000001 + 7

    def values_out_of_index(self, ix):
        return self.values_in(ix)


# ---------------------------------------------------------------------------------------------------------------------
# runs: unique-consecutive, run lengths, reduce by run, scan by key
# ---------------------------------------------------------------------------------------------------------------------
class Runs:
    """key(i) = (3 i) >> 4: runs of 5, 5 and 6 elements.  Run v starts at start(v) = ceil(16 v / 3) = (16 v + 2) // 3."""

    def __init__(self, n):
        self.n = n
        self.num_runs = ((3 * (n - 1)) >> 4) + 1 if n else 0

    def key(self, i):
        return (3 * i) >> 4

    @staticmethod
    def start(v):
        return (16 * v + 2) // 3

    def end(self, v):
        return torch.clamp(self.start(v + 1), max=self.n)

    def offsets(self, r):
        """r <= num_runs: the start of run r, n at r == num_runs"""
        return torch.clamp(self.start(r), max=self.n)

    def counts(self, v):
        return self.end(v) - self.start(v)

    def sum_of_positions(self, v):
        a, b = self.start(v), self.end(v)
        return (a + b - 1) * (b - a) // 2

    def min_of_positions(self, v):
        return self.start(v)

    def max_of_positions(self, v):
        return self.end(v) - 1

    def count_so_far(self, i):
        """the inclusive sum scan by key of ones"""
        return i - self.start(self.key(i)) + 1


# ---------------------------------------------------------------------------------------------------------------------
# scans
# ---------------------------------------------------------------------------------------------------------------------
def scan_sum_in(i):
    return (i % 7) + 1


def scan_sum_out(i):
    """the inclusive sum of scan_sum_in; a u32 scan wraps, which the comparison of the low 32 bits accounts for"""
    tri = torch.tensor(TRI7, dtype=torch.int64, device=i.device)
    return 28 * (i // 7) + tri[i % 7]


def scan_sum_exclusive_out(init):
    return lambda i: init + torch.where(i > 0, scan_sum_out(torch.clamp(i - 1, min=0)), torch.zeros_like(i))


def scan_max_in(i):
    return i ^ 1


def scan_max_out(i):
    return i | 1


def scan_min_in(n):
    return lambda i: n - (i ^ 1)


def scan_min_out(n):
    return lambda i: n - (i | 1)


# ---------------------------------------------------------------------------------------------------------------------
# histograms
# ---------------------------------------------------------------------------------------------------------------------
def bincount_in(n, bins):
    p = Perm(n)
    return lambda i: p(i) % bins


def bincount_out(n, bins):
    return lambda b: n // bins + (b < n % bins).to(torch.int64)


def edges(n, bins):
    """bins + 1 rising edges over P's range that start above 0 and end below n (keys outside are ignored), with one repeated edge
    (an empty bin) when there are at least 4 bins"""
    def form(b):
        e = 3 + (b * (n - 10)) // bins
        if bins >= 4:
            e = torch.where(b == 2, 3 + (1 * (n - 10)) // bins, e)
        return e
    return form


def histogram_range_out(n, bins):
    """keys P(i) are 0 .. n - 1 once each: a bin's count is the width of its interval clipped to [0, n)"""
    e = edges(n, bins)
    return lambda b: torch.clamp(e(b + 1), 0, n) - torch.clamp(e(b), 0, n)


# ---------------------------------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------------------------------
def flags_in(i):
    return (i % 3 == 0).to(torch.int64)


def flagged_count(n):
    return (n + 2) // 3


def flagged_index_out(j):
    return 3 * j


def rejected_index_out(n):
    """partition: the k-th rejected element (k = j - count) is the k-th i with i mod 3 != 0"""
    c = flagged_count(n)
    return lambda j: 3 * ((j - c) // 2) + 1 + (j - c) % 2


# ---------------------------------------------------------------------------------------------------------------------
# merge and set operations
# ---------------------------------------------------------------------------------------------------------------------
def merge_in(i):
    """both inputs: pairs of equal keys, so ties within an input and across the inputs"""
    return 2 * (i >> 1)


class Merge:
    """a[i] = b[i] = 2 (i >> 1).  While both inputs last (j < 4 * (min(na, nb) // 2)) every key 2 q fills four slots: a[2q], a[2q + 1],
    b[2q], b[2q + 1].  Behind that the longer input follows alone, after the odd element of the shorter one."""

    def __init__(self, na, nb):
        self.na, self.nb = na, nb
        self.both = 4 * (min(na, nb) // 2)

    def source(self, j):
        """the position in A || B of out[j]"""
        na, nb, m = self.na, self.nb, min(self.na, self.nb)
        q, r = j // 4, j % 4
        body = torch.where(r < 2, 2 * q + r, na + 2 * q + r - 2)
        t = j - self.both          # the tail: what is left of A is a[m2 ..], of B b[m2 ..], m2 = 2 (m // 2)
        m2 = 2 * (m // 2)
        ra, rb = na - m2, nb - m2
        if ra >= rb:
            # A is the longer one; B has rb in {0, 1} elements left, with key m2 == a[m2]'s: it comes behind a's pair (or a's single element)
            pair = min(2, ra)
            tail = torch.where(t < pair, m2 + t, torch.where(t < pair + rb, na + m2 + (t - pair), m2 + t - rb))
        else:
            # B is the longer one; A has ra in {0, 1} elements left: it comes first
            tail = torch.where(t < ra, m2 + t, na + m2 + (t - ra))
        return torch.where(j < self.both, body, tail)

    def keys_out(self, j):
        s = self.source(j)
        return merge_in(torch.where(s < self.na, s, s - self.na))


class SetOps:
    """a[i] = 2 i (i < na), b[i] = 3 i (i < nb): no duplicates.  With La = 2 na and Lb = 3 nb (both < 2^32) a holds the even numbers
    below La, b the multiples of 3 below Lb.  out[j] for the four operations, each by residues mod 6, valid while j < count()."""

    def __init__(self, na, nb):
        assert 2 * na < (1 << 32) and 3 * nb < (1 << 32)
        # the closed forms below hold while both inputs reach as far as the result is read: keep the ranges nested a-in-b or b-in-a simply
        # by cutting every form at L = min(La, Lb) and appending the longer input's own tail
        self.na, self.nb = na, nb
        self.La, self.Lb = 2 * na, 3 * nb
        self.L = min(self.La, self.Lb)

    @staticmethod
    def _below(L, residues):
        """how many x < L have x mod 6 in residues"""
        return sum((L - r + 5) // 6 for r in residues if L > r)

    @staticmethod
    def _pick(j, residues):
        k = len(residues)
        res = torch.tensor(residues, dtype=torch.int64, device=j.device)
        return 6 * (j // k) + res[j % k]

    def _tail_a(self):
        return self.La > self.Lb

    def count(self, op):
        L = self.L
        c = self._below(L, {"intersection": (0,), "union": (0, 2, 3, 4), "difference": (2, 4), "symmetric_difference": (2, 3, 4)}[op])
        extra_a = self._below(self.La, (0, 2, 4)) - self._below(L, (0, 2, 4))      # a's elements at L and beyond: in no b
        extra_b = self._below(self.Lb, (0, 3)) - self._below(L, (0, 3))
        if op == "intersection":
            return c
        if op == "difference":
            return c + extra_a
        return c + extra_a + extra_b

    def keys_out(self, op):
        residues = {"intersection": (0,), "union": (0, 2, 3, 4), "difference": (2, 4), "symmetric_difference": (2, 3, 4)}[op]
        c = self._below(self.L, residues)
        a_tail0 = self._below(self.L, (0, 2, 4))   # the first index of a at or beyond L
        b_tail0 = self._below(self.L, (0, 3))

        def form(j):
            body = self._pick(j, residues)
            t = j - c
            if self._tail_a() and op != "intersection":
                tail = 2 * (a_tail0 + t)
            elif not self._tail_a() and op in ("union", "symmetric_difference"):
                tail = 3 * (b_tail0 + t)
            else:
                tail = body
            return torch.where(j < c, body, tail)
        return form

    def source(self, op):
        """the position in A || B of out[j]: even keys below La come from A (a multiple of 6 is in both: intersection and union keep
        A's), odd multiples of 3 and everything at La and beyond from B"""
        k = self.keys_out(op)

        def form(j):
            x = k(j)
            return torch.where((x % 2 == 0) & (x < self.La), x // 2, self.na + x // 3)
        return form


# ---------------------------------------------------------------------------------------------------------------------
# sorted search
# ---------------------------------------------------------------------------------------------------------------------
def haystack(i):
    """h[i] = 3 (i >> 1): every multiple of 3 twice"""
    return 3 * (i >> 1)


def search_left(m):
    return lambda q: torch.clamp(2 * ((q + 2) // 3), max=m)


def search_right(m):
    return lambda q: torch.clamp(2 * (q // 3 + 1), max=m)


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
class Rows32:
    """rows of 32 columns: key[r, c] = r + ((5 c + r) mod 32) sorts to r + c with index ((c - r) 13) mod 32 (5 * 13 = 65 = 1 mod 32).
    Flat index f = r * 32 + c.  Descending: column c holds what ascending column 31 - c holds."""
    cols = 32

    def __init__(self, rows, order=ASC):
        self.rows, self.order = rows, order

    def keys_in(self, f):
        r, c = f >> 5, f & 31
        return r + ((5 * c + r) & 31)

    def _c(self, f):
        c = f & 31
        return c if self.order == ASC else 31 - c

    def keys_out(self, f):
        return (f >> 5) + self._c(f)

    def index_out(self, f):
        return ((self._c(f) - (f >> 5)) * 13) & 31


class RowsPrime:
    """rows of a prime number of columns: key[r, c] = r + ((mult c + r) mod cols) sorts to r + c; the index is pinned by the gather
    property alone, the keys of a row being distinct."""

    def __init__(self, rows, cols, mult=PRIME_A, order=ASC, stride=None):
        assert mult % cols != 0
        self.rows, self.cols, self.mult, self.order, self.stride = rows, cols, mult % cols, order, stride or cols

    def keys_in_at(self, r, c):
        return r + ((self.mult * c + r) % self.cols)

    def keys_in_strided(self, e):
        """element e of the strided input; the padding between cols and stride holds a poison key"""
        r, c = e // self.stride, e % self.stride
        return torch.where(c < self.cols, self.keys_in_at(r, torch.clamp(c, max=self.cols - 1)), torch.full_like(e, 0x7fffffff))

    def keys_out(self, f):
        r, c = f // self.cols, f % self.cols
        return r + (c if self.order == ASC else self.cols - 1 - c)

    def key_at_index(self, f, ix):
        """the input key of row(f) at column ix"""
        return self.keys_in_at(f // self.cols, ix)


# ---------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------
class Segments:
    """S segments in periods of 8 with the lengths of `pattern` (empty ones, one per class of the plan), optionally one long segment in
    front.  off(s) is a closed form; the segment of an element is found by dividing by the period's length and a search in the
    pattern's 8 prefix sums.  The local key is (local A) mod len, A a prime above every len: a permutation of 0 .. len - 1, so the
    sorted keys are the local positions j - off[seg(j)].  dup: keys >> 1, ties inside every segment."""

    PATTERN = (0, 1, 2, 37, 0, 300, 4096, 5)

    def __init__(self, periods, long_first=0, pattern=PATTERN, order=ASC, dup=0):
        self.pattern, self.periods, self.long_first, self.order, self.dup = pattern, periods, long_first, order, dup
        self.pre = [sum(pattern[:k]) for k in range(9)]
        self.plen = self.pre[8]
        self.lead = 1 if long_first else 0
        self.S = 8 * periods + self.lead
        self.n = long_first + periods * self.plen
        self.max_segment = max(max(pattern), long_first)
        assert self.max_segment < PRIME_A and self.n < (1 << 32)

    def offsets(self, s):
        """s <= S"""
        t = s - self.lead
        pre = torch.tensor(self.pre, dtype=torch.int64, device=s.device)
        body = self.long_first + (t // 8) * self.plen + pre[torch.clamp(t, min=0) % 8]
        return torch.where(t < 0, torch.zeros_like(s), body)

    def locate(self, e):
        """(offset of the element's segment, its length) for element e"""
        t = e - self.long_first
        tt = torch.clamp(t, min=0)
        per, x = tt // self.plen, tt % self.plen
        pre = torch.tensor(self.pre[1:], dtype=torch.int64, device=e.device)
        k = torch.bucketize(x, pre, right=True)                       # the slot whose [pre[k], pre[k + 1]) holds x
        pre0 = torch.tensor(self.pre, dtype=torch.int64, device=e.device)
        off = self.long_first + per * self.plen + pre0[k]
        ln = pre0[k + 1] - pre0[k]
        if self.long_first:
            inlong = t < 0
            off = torch.where(inlong, torch.zeros_like(e), off)
            ln = torch.where(inlong, torch.full_like(e, self.long_first), ln)
        return off, ln

    def keys_in(self, e):
        off, ln = self.locate(e)
        return (((e - off) * PRIME_A) % ln) >> self.dup

    def keys_out(self, e):
        off, ln = self.locate(e)
        loc = e - off
        return (loc if self.order == ASC else ln - 1 - loc) >> self.dup

    def segment_start(self, e):
        return self.locate(e)[0]


# ---------------------------------------------------------------------------------------------------------------------
# groups: unique of unsorted keys, reduce by key
# ---------------------------------------------------------------------------------------------------------------------
class Groups:
    """key(i) = Pm(i mod m), Pm a permutation of 0 .. m - 1: m distinct keys, key v at the positions Pm^-1(v) + t m.  So the sorted
    unique keys are 0 .. m - 1, the first position of key v is Pm^-1(v), its count is the number of i < n with i mod m == Pm^-1(v),
    the inverse index of element i is key(i), and the sum of the positions of key v is c x + m c (c - 1) / 2 with x the first and c the count."""

    def __init__(self, n, m):
        assert 0 < m <= n
        self.n, self.m, self.p = n, m, Perm(m)

    def key(self, i):
        return self.p(i % self.m)

    def first_index(self, v):
        return self.p.inv(v)

    def counts(self, v):
        return self.n // self.m + (self.p.inv(v) < self.n % self.m).to(torch.int64)

    def sum_of_positions(self, v):
        x, c = self.first_index(v), self.counts(v)
        return c * x + self.m * (c * (c - 1) // 2)
