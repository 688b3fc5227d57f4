"""Sorted search: what can be checked without a GPU -- the symbol and its signature, the defines and the two knobs in the header, the
refusals that need no device (a null handle; what Pprims.searchSorted refuses itself), the oracle the GPU tests use
(tests/search_oracle.py) against a plain counting loop, and the facade's host path (tests/demo/search_demo --host) against that
oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from search_oracle import ASC, BY_NAME, DESC, LEFT, RIGHT, SPECIALS, TYPE_IDS, codes, decode, is_sorted, search_oracle, sort_bits

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "search_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
DEMO_SIZES, DEMO_DUMPED = 6, 4   # sizes, and those small enough to be dumped
DEMO_PATTERNS = 3


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_search_symbol_is_bound_with_the_declared_signature(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_search_sorted_typed\(adlhip_device\* dev, int key_type, int order, int side,\s+"
                     r"const void\* d_sorted, size_t m, const void\* d_needles, size_t n,\s+"
                     r"uint32_t\* d_pos_out\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    sig = (I, [VP, I, I, I, VP, SZ, VP, SZ, VP])
    assert _lib.SIGNATURES["adlhip_search_sorted_typed"] == sig
    fn = getattr(built, "adlhip_search_sorted_typed")
    assert fn.argtypes == sig[1] and fn.restype is I
    assert re.search(r"#define ADLHIP_SEARCH_LEFT 0\b", header) and re.search(r"#define ADLHIP_SEARCH_RIGHT 1\b", header)
    assert re.search(r"#define ADLHIP_SEARCH_TILE 2048\b", header)
    assert '"debug.search_lds_keys"' in header and '"debug.search_grid"' in header
    # the header states the relation to the merge, what holds for a sequence that is not sorted, and that no scratch function exists
    assert "i + LEFT_B(A[i])" in header and "j + RIGHT_A(B[j])" in header and "NOT sorted" in header
    assert "adlhip_search_sorted_scratch_bytes" not in header and not any("search" in k and "scratch" in k for k in _lib.SIGNATURES)


def test_null_handle_is_rejected_by_the_search_entry_point(built):
    rc = built.adlhip_search_sorted_typed(None, 0, 0, 0, None, 10, None, 10, None)
    assert rc == 1   # ADLHIP_FAILURE
    assert b"null device handle" in built.adlhip_last_error()


class _Buf:
    """what Pprims.searchSorted looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_search_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    s, x, pos = _Buf(np.float32, 100), _Buf(np.float32, 50), _Buf(np.uint32, 50)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.searchSorted(None, s, x, pos, 100, 50)
    for args in ((None, x, pos), (s, None, pos), (s, x, None)):
        with pytest.raises(AdlHipError, match="are required"):
            p.searchSorted(dev, *args, 100, 50)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.searchSorted(dev, _Buf(bad, 100), _Buf(bad, 50), pos, 100, 50)
    with pytest.raises(AdlHipError, match="sortedKeys is float32, needles int32"):
        p.searchSorted(dev, s, _Buf(np.int32, 50), pos, 100, 50)
    for m, n in ((-1, 50), (101, 50), (100, -1), (100, 51)):
        with pytest.raises(AdlHipError, match="outside"):
            p.searchSorted(dev, s, x, pos, m, n)
    with pytest.raises(AdlHipError, match="m = 4294967296; fewer than 2\\^32"):
        p.searchSorted(dev, _Buf(np.uint32, 1 << 32), _Buf(np.uint32, 50), pos, 1 << 32, 50)
    with pytest.raises(AdlHipError, match="n = 4294967296; fewer than 2\\^32"):
        p.searchSorted(dev, _Buf(np.uint32, 100), _Buf(np.uint32, 1 << 32), _Buf(np.uint32, 1 << 32), 100, 1 << 32)
    with pytest.raises(AdlHipError, match="posOut must be a uint32 buffer of 50 elements"):
        p.searchSorted(dev, s, x, _Buf(np.uint32, 49), 100, 50)
    with pytest.raises(AdlHipError, match="posOut must be a uint32 buffer"):
        p.searchSorted(dev, s, x, _Buf(np.int64, 50), 100, 50)


def test_torch_sorter_has_the_search():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.searchsorted) and callable(TorchSorter.bucketize)
    doc = TorchSorter.searchsorted.__doc__
    assert "torch.searchsorted" in doc and "totalOrder" in doc and "-0" in doc and "NaN" in doc
    assert "sorter=" in doc and "batched" in doc and "Nothing reaches the host" in doc
    assert "torch.bucketize" in TorchSorter.bucketize.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a plain counting loop
# ---------------------------------------------------------------------------------------------
def _typed_less(name, a, b):
    """a sorts before b (ascending), stated per type and independently of encode(): integers by value; floats by sign, then by
    magnitude bits"""
    w = 4 if name.endswith("32") else 8
    if name[0] == "u":
        return a < b
    sign = 1 << (8 * w - 1)
    if name[0] == "i":
        sa, sb = (a - (1 << (8 * w)) if a & sign else a), (b - (1 << (8 * w)) if b & sign else b)
        return sa < sb
    na, nb = bool(a & sign), bool(b & sign)
    if na != nb:
        return na
    ma, mb = a & (sign - 1), b & (sign - 1)
    return ma > mb if na else ma < mb


def _count(name, order, side, seq, needles):
    """counted, not searched: the elements in front of the needle (RIGHT: not behind it)"""
    before = (lambda x, y: _typed_less(name, y, x)) if order == DESC else (lambda x, y: _typed_less(name, x, y))
    seq = seq.tolist()
    if side == LEFT:
        return [sum(1 for e in seq if before(e, x)) for x in needles.tolist()]
    return [sum(1 for e in seq if not before(x, e)) for x in needles.tolist()]


def _inputs(name, rng):
    """(sequence, needles) pairs of bit patterns, the sequence unsorted: random bits with every special value in both, runs of equal
    elements, an empty sequence, one element"""
    udt = BY_NAME[name][3]
    w = np.dtype(udt).itemsize
    sp = SPECIALS[w]

    def rnd(n):
        return np.frombuffer(rng.bytes(w * n), dtype=udt).copy()
    yield np.concatenate([sp, rnd(40), sp[::2]]), np.concatenate([rnd(25), sp, sp[::3]])
    yield np.full(17, sp[3], udt), np.concatenate([sp, np.full(3, sp[3], udt)])          # one run
    yield np.zeros(0, udt), np.concatenate([sp, rnd(5)])                                 # an empty sequence
    yield sp[rng.integers(0, 3, size=50)], np.concatenate([sp[:3], sp, rnd(7)])          # three values, long runs
    yield rnd(1), np.concatenate([rnd(3), sp])
    yield np.repeat(rnd(9), 5), rnd(4)


@pytest.mark.parametrize("side", [LEFT, RIGHT], ids=["left", "right"])
@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_search_oracle_agrees_with_a_counting_loop(name, order, side):
    rng = np.random.default_rng(31 + BY_NAME[name][1])
    for seq, needles in _inputs(name, rng):
        seq = sort_bits(seq, name, order)
        assert is_sorted(seq, name, order)
        needles = np.concatenate([needles, seq])                      # every element of the sequence itself
        c = codes(seq, name, order)                                   # and every element's code +- 1, where that exists
        one = c.dtype.type(1)
        needles = np.concatenate([needles, decode(c[c != ~c.dtype.type(0)] + one, name, order), decode(c[c != 0] - one, name, order)])
        got = search_oracle(seq, needles, name, order, side)
        assert got.dtype == np.uint32 and got.tolist() == _count(name, order, side, seq, needles), (name, order, side, seq.size)
        assert (got <= seq.size).all()


def test_decode_inverts_codes():
    for name in TYPE_IDS:
        sp = SPECIALS[np.dtype(BY_NAME[name][3]).itemsize]
        for order in (ASC, DESC):
            assert np.array_equal(decode(codes(sp, name, order), name, order), sp)


def test_oracle_on_specials_by_hand():
    # totalOrder: -0 below +0; -NaN first, +NaN last
    seq = sort_bits(np.array([0x00000000, 0x80000000, 0x7fc00000, 0xffc00000, 0x3f800000], np.uint32), "f32")
    assert seq.tolist() == [0xffc00000, 0x80000000, 0x00000000, 0x3f800000, 0x7fc00000]
    x = np.array([0x80000000, 0x00000000, 0xffc00000, 0x7fc00000], np.uint32)
    assert search_oracle(seq, x, "f32", ASC, LEFT).tolist() == [1, 2, 0, 4]
    assert search_oracle(seq, x, "f32", ASC, RIGHT).tolist() == [2, 3, 1, 5]
    assert search_oracle(seq[::-1].copy(), x, "f32", DESC, LEFT).tolist() == [3, 2, 4, 0]
    # a run: LEFT in front of it, RIGHT behind it
    run = np.full(9, 7, np.uint64)
    assert search_oracle(run, run[:1], "i64", ASC, LEFT).tolist() == [0] and search_oracle(run, run[:1], "i64", ASC, RIGHT).tolist() == [9]
    # integer extremes
    seq = sort_bits(np.array([0x80000000, 0x7fffffff, 0, 0xffffffff], np.uint32), "i32")
    assert seq.tolist() == [0x80000000, 0xffffffff, 0, 0x7fffffff]
    assert search_oracle(seq, np.array([0x80000000, 0x7fffffff], np.uint32), "i32", ASC, RIGHT).tolist() == [1, 4]
    assert search_oracle(np.zeros(0, np.uint32), np.array([5], np.uint32), "u32").tolist() == [0]


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def test_search_demo_host_path_matches_the_oracle(built):
    r = subprocess.run([DEMO, "--host", "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    ok = [ln for ln in lines if ln.startswith("[")]
    per_size = 2 * 2 * DEMO_PATTERNS * len(TYPE_IDS)
    assert len(ok) == DEMO_SIZES * per_size, len(ok)
    assert all(ln.startswith("[ OK ] Search.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == DEMO_DUMPED * per_size   # the cases with m and n <= 1000
    seen = set()
    hits = 0
    for ln in dumps:
        head, rest = ln.split(":", 1)
        _, _, kname, oname, sname, m, n = head.split()
        m, n, order, side = int(m), int(n), {"asc": ASC, "desc": DESC}[oname], {"left": LEFT, "right": RIGHT}[sname]
        parts = rest.split("|")
        kudt = BY_NAME[kname][3]
        seq, needles = _bits(parts[0], kudt), _bits(parts[1], kudt)
        assert seq.size == m and needles.size == n
        assert is_sorted(seq, kname, order), ln[:80]
        assert np.array_equal(_bits(parts[2], np.uint32), search_oracle(seq, needles, kname, order, side)), ln[:80]
        seen.add((kname, oname, sname))
        hits += bool(m and np.intersect1d(seq, needles).size)
    assert len(seen) == 4 * len(TYPE_IDS)
    assert hits > len(dumps) // 2, "the demo's needles must meet equal elements of the sequence"


def test_facade_exports_the_search(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for k in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" W void Tahoe::Pprims::searchSorted<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const&, "
                         r"adl::Buffer<unsigned int>&, int, int, bool, bool\)" % tuple(re.escape(x) for x in (k, k, k)), out), k
