"""Merge of sorted sequences: what can be checked without a GPU -- the two symbols and their signatures, the knob and the tile in the
header, the refusals that need no device (a null handle; what Pprims.mergeKeys / mergePairs refuse themselves), the oracle the GPU
tests use (tests/merge_oracle.py) against a plain two-pointer loop in which a tie takes A, and the facade's host path
(tests/demo/merge_demo --host) against that oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from merge_oracle import ASC, BY_NAME, DESC, SPECIALS, TYPE_IDS, codes, is_sorted, merge_oracle, sort_bits
from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "merge_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
DEMO_SIZES, DEMO_DUMPED = 6, 4   # sizes, and those small enough to be dumped
DEMO_PATTERNS = 3
DEMO_TYPES = (("u32", "none"), ("i32", "f64"), ("f32", "i32"), ("u64", "f32"), ("i64", "none"), ("f64", "i64"))


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_merge_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_merge_scratch_bytes\(adlhip_device\* dev, int key_type, int value_bytes, size_t na, size_t nb, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_merge_typed\(adlhip_device\* dev, int key_type, int order,\s+"
                     r"const void\* d_keys_a, const void\* d_vals_a_or_null, size_t na,\s+"
                     r"const void\* d_keys_b, const void\* d_vals_b_or_null, size_t nb,\s+"
                     r"int value_bytes, void\* d_keys_out_or_null, void\* d_vals_out_or_null, uint32_t\* d_index_out_or_null,\s+"
                     r"void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_merge_scratch_bytes": (I, [VP, I, I, SZ, SZ, ctypes.POINTER(SZ)]),
        "adlhip_merge_typed": (I, [VP, I, I, VP, VP, SZ, VP, VP, SZ, I, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.merge_grid"' in header
    assert re.search(r"#define ADLHIP_MERGE_TILE 2048\b", header)
    # the header states the work formula and what holds for inputs that are not sorted
    assert "4 x (tiles + 1) rounded up to 256" in header and "NOT sorted" in header


def test_null_handle_is_rejected_by_the_merge_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_merge_scratch_bytes(None, 0, 0, 10, 10, ctypes.byref(sz)),
               lib.adlhip_merge_typed(None, 0, 0, None, None, 10, None, None, 10, 0, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.mergeKeys looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_merge_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    a, b, out = _Buf(np.float32, 100), _Buf(np.float32, 50), _Buf(np.float32, 150)
    va, vb, vout = _Buf(np.int64, 100), _Buf(np.int64, 50), _Buf(np.int64, 150)

    with pytest.raises(AdlHipError, match="needs a device"):
        p.mergeKeys(None, a, b, out, 100, 50)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.mergePairs(None, a, va, b, vb, out, vout, 100, 50)
    with pytest.raises(AdlHipError, match="both inputs are required"):
        p.mergeKeys(dev, a, None, out, 100, 0)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.mergeKeys(dev, _Buf(bad, 100), _Buf(bad, 50), _Buf(bad, 150), 100, 50)
        with pytest.raises(AdlHipError, match="unsupported values type"):
            p.mergePairs(dev, a, _Buf(bad, 100), b, _Buf(bad, 50), out, _Buf(bad, 150), 100, 50)
    with pytest.raises(AdlHipError, match="a is float32, b int32"):
        p.mergeKeys(dev, a, _Buf(np.int32, 50), out, 100, 50)
    for na, nb in ((-1, 50), (101, 50), (100, -1), (100, 51)):
        with pytest.raises(AdlHipError, match="outside"):
            p.mergeKeys(dev, a, b, out, na, nb)
    with pytest.raises(AdlHipError, match="fewer than 2\\^32"):
        p.mergeKeys(dev, _Buf(np.uint32, 1 << 31), _Buf(np.uint32, 1 << 31), _Buf(np.uint32, 1 << 32), 1 << 31, 1 << 31)
    with pytest.raises(AdlHipError, match="out must hold"):
        p.mergeKeys(dev, a, b, _Buf(np.float32, 149), 100, 50)
    with pytest.raises(AdlHipError, match="out must hold"):
        p.mergeKeys(dev, a, b, _Buf(np.int32, 150), 100, 50)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.mergeKeys(dev, a, b, None, 100, 50)
    with pytest.raises(AdlHipError, match="valuesA, valuesB and valuesOut are required"):
        p.mergePairs(dev, a, va, b, None, out, vout, 100, 50)
    with pytest.raises(AdlHipError, match="the values are int64, int32 and int64"):
        p.mergePairs(dev, a, va, b, _Buf(np.int32, 50), out, vout, 100, 50)
    with pytest.raises(AdlHipError, match="the values must hold"):
        p.mergePairs(dev, a, va, b, vb, out, _Buf(np.int64, 149), 100, 50)
    with pytest.raises(AdlHipError, match="indexOut must be"):
        p.mergeKeys(dev, a, b, out, 100, 50, indexOut=_Buf(np.uint32, 149))
    with pytest.raises(AdlHipError, match="indexOut must be"):
        p.mergeKeys(dev, a, b, out, 100, 50, indexOut=_Buf(np.int64, 150))


def test_torch_sorter_has_the_merge():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.merge)
    doc = TorchSorter.merge.__doc__
    assert "torch.sort(torch.cat((a, b))" in doc and "stable=True" in doc and "without a copy" in doc


# ---------------------------------------------------------------------------------------------
# the oracle against a plain loop
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


def _two_pointer(name, order, a, b):
    """positions in a || b of the merge in which b goes first only where it is strictly in front: a tie takes A"""
    before = (lambda x, y: _typed_less(name, y, x)) if order == DESC else (lambda x, y: _typed_less(name, x, y))
    a, b = a.tolist(), b.tolist()
    i = j = 0
    out = []
    while i < len(a) or j < len(b):
        if i >= len(a) or (j < len(b) and before(b[j], a[i])):
            out.append(len(a) + j)
            j += 1
        else:
            out.append(i)
            i += 1
    return out


def _inputs(name, rng):
    """(a, b) pairs of bit patterns, unsorted: random bits with every special value in both, all ties, one side empty, few values"""
    udt = BY_NAME[name][3]
    w = np.dtype(udt).itemsize
    sp = SPECIALS[w]

    def rnd(n):
        return np.frombuffer(rng.bytes(w * n), dtype=udt).copy()
    yield np.concatenate([sp, rnd(40), sp[::2]]), np.concatenate([rnd(25), sp, sp[::3]])
    yield np.full(17, sp[3], udt), np.full(9, sp[3], udt)                     # all ties
    yield np.zeros(0, udt), np.concatenate([sp, rnd(5)])                      # one side empty
    yield np.concatenate([sp, rnd(5)]), np.zeros(0, udt)
    yield np.zeros(0, udt), np.zeros(0, udt)
    yield sp[rng.integers(0, 3, size=50)], sp[rng.integers(0, 3, size=31)]    # three values, long runs of ties
    yield rnd(1), rnd(1)


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_merge_oracle_agrees_with_a_two_pointer_loop(name, order):
    rng = np.random.default_rng(29 + BY_NAME[name][1])
    for a, b in _inputs(name, rng):
        a, b = sort_bits(a, name, order), sort_bits(b, name, order)
        assert is_sorted(a, name, order) and is_sorted(b, name, order)
        loop_sorted = all(not _typed_less(name, *((x, y) if order == DESC else (y, x))) for x, y in zip(a.tolist(), a.tolist()[1:]))
        assert loop_sorted, "sort_bits and the per-type order disagree"
        va = np.arange(a.size, dtype=np.uint64) * np.uint64(3)
        vb = np.arange(b.size, dtype=np.uint64) * np.uint64(5) + np.uint64(1)
        index, keys, vals = merge_oracle(a, b, name, order, va, vb)
        want = _two_pointer(name, order, a, b)
        assert index.dtype == np.uint32 and index.tolist() == want, (name, order, a.size, b.size)
        cat, vcat = np.concatenate([a, b]), np.concatenate([va, vb])
        assert keys.tolist() == [int(cat[i]) for i in want] and vals.tolist() == [int(vcat[i]) for i in want]
        assert keys.dtype == a.dtype and is_sorted(keys, name, order)
        # stability: the elements of each input keep their order
        ia, ib = index[index < a.size], index[index >= a.size]
        assert (np.diff(ia.astype(np.int64)) > 0).all() and (np.diff(ib.astype(np.int64)) > 0).all()


def test_oracle_ties_take_a_in_both_orders_and_all_ties_give_the_identity():
    a = np.array([1, 5, 5, 9], np.uint32)
    b = np.array([5, 5, 9, 10], np.uint32)
    index, keys, _ = merge_oracle(a, b, "u32", ASC)
    assert index.tolist() == [0, 1, 2, 4, 5, 3, 6, 7] and keys.tolist() == [1, 5, 5, 5, 5, 9, 9, 10]
    index, keys, _ = merge_oracle(a[::-1], b[::-1], "u32", DESC)
    assert index.tolist() == [4, 0, 5, 1, 2, 6, 7, 3] and keys.tolist() == [10, 9, 9, 5, 5, 5, 5, 1]
    same = np.full(6, 0x7fc00000, np.uint32)
    for order in (ASC, DESC):
        assert merge_oracle(same[:4], same[:2], "f32", order)[0].tolist() == list(range(6))
    # totalOrder: -0 is in front of +0 ascending, behind it descending
    z = np.array([0x80000000], np.uint32), np.array([0x00000000], np.uint32)
    assert merge_oracle(z[1], z[0], "f32", ASC)[0].tolist() == [1, 0]
    assert merge_oracle(z[1], z[0], "f32", DESC)[0].tolist() == [0, 1]
    assert (codes(SPECIALS[4], "i32", DESC) == ~codes(SPECIALS[4], "i32", ASC)).all()


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def test_merge_demo_host_path_matches_the_oracle(built):
    r = subprocess.run([DEMO, "--host", "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    ok = [ln for ln in lines if ln.startswith("[")]
    per_size = 2 * DEMO_PATTERNS * len(DEMO_TYPES)
    assert len(ok) == DEMO_SIZES * per_size, len(ok)
    assert all(ln.startswith("[ OK ] Merge.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == DEMO_DUMPED * per_size   # the cases with na + nb <= 1000
    seen = set()
    ties = 0
    for ln in dumps:
        head, rest = ln.split(":", 1)
        _, _, kname, vname, oname, na, nb = head.split()
        na, nb, order = int(na), int(nb), {"asc": ASC, "desc": DESC}[oname]
        parts = rest.split("|")
        kudt = BY_NAME[kname][3]
        a, b = _bits(parts[0], kudt), _bits(parts[1], kudt)
        assert a.size == na and b.size == nb
        assert is_sorted(a, kname, order) and is_sorted(b, kname, order), ln[:80]
        va = vb = None
        if vname != "none":
            vudt = BY_NAME[vname][3]
            va, vb = _bits(parts[2], vudt), _bits(parts[3], vudt)
            assert va.size == na and vb.size == nb
        index, keys, vals = merge_oracle(a, b, kname, order, va, vb)
        assert np.array_equal(_bits(parts[4], kudt), keys) and np.array_equal(_bits(parts[6], np.uint32), index), ln[:80]
        if vname != "none":
            assert np.array_equal(_bits(parts[5], BY_NAME[vname][3]), vals), ln[:80]
        seen.add((kname, vname, oname))
        ties += bool(na and nb and np.intersect1d(a, b).size)
    assert len(seen) == 2 * len(DEMO_TYPES)
    assert ties > len(dumps) // 4, "the demo's cases must make keys of A meet equal keys of B"


def test_facade_exports_the_merges(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for k in names:
        for v in names:
            assert re.search(r" W void Tahoe::Pprims::mergePairs<%s, %s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const\*, "
                             r"adl::Buffer<%s> const&, adl::Buffer<%s> const\*, adl::Buffer<%s>&, adl::Buffer<%s>\*, adl::Buffer<unsigned int>\*, "
                             r"int, int, bool\)" % tuple(re.escape(x) for x in (k, v, k, v, k, v, k, v)), out), (k, v)
