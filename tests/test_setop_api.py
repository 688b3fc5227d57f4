"""Set operations on sorted sequences: what can be checked without a GPU -- the two symbols and their signatures, the knob, the tile
and the operations in the header, the refusals that need no device (a null handle; what Pprims.setOp refuses itself), the oracle the
GPU tests use (tests/setop_oracle.py) against two independent restatements -- a collections.Counter multiset for the key multiset,
thrust's two-pointer loops for the exact elements and their order -- and the facade's host path (tests/demo/setop_demo --host)
against that oracle."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from setop_oracle import (ASC, BY_NAME, DESC, DIFFERENCE, INTERSECTION, OP_IDS, OPS, SPECIALS, SYMMETRIC_DIFFERENCE, TYPE_IDS, UNION, capacity,
                          is_sorted, merge_oracle, setop_oracle, sort_bits)
from test_merge_api import _Buf, _inputs, _typed_less

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "setop_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
DEMO_SIZES, DEMO_DUMPED = 5, 3   # sizes, and those small enough to be dumped
DEMO_PATTERNS = 2
DEMO_TYPES = (("u32", "none"), ("i32", "f64"), ("f32", "i32"), ("u64", "f32"), ("i64", "none"), ("f64", "i64"))
ALL_OPS = (INTERSECTION, UNION, DIFFERENCE, SYMMETRIC_DIFFERENCE)


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_set_op_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_set_op_scratch_bytes\(adlhip_device\* dev, int key_type, int value_bytes, size_t na, size_t nb, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_set_op_typed\(adlhip_device\* dev, int key_type, int order, int op,\s+"
                     r"const void\* d_keys_a, const void\* d_vals_a_or_null, size_t na,\s+"
                     r"const void\* d_keys_b, const void\* d_vals_b_or_null, size_t nb,\s+"
                     r"int value_bytes, void\* d_keys_out_or_null, void\* d_vals_out_or_null, uint32_t\* d_index_out_or_null,\s+"
                     r"uint32_t\* d_num_out, void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_set_op_scratch_bytes": (I, [VP, I, I, SZ, SZ, ctypes.POINTER(SZ)]),
        "adlhip_set_op_typed": (I, [VP, I, I, I, VP, VP, SZ, VP, VP, SZ, I, VP, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.setop_grid"' in header
    assert re.search(r"#define ADLHIP_SETOP_TILE 2048\b", header)
    for name, value in (("INTERSECTION", 0), ("UNION", 1), ("DIFFERENCE", 2), ("SYMMETRIC_DIFFERENCE", 3)):
        assert re.search(r"#define ADLHIP_SETOP_%s %d\b" % (name, value), header)
        assert OP_IDS[name.lower()] == value
    # the header states the work formula and what holds for inputs that are not sorted
    assert "4 x 8 x CUs rounded up to 256" in header and "4 x (tiles + 1) rounded up to 256" in header and "*d_num_out <= cap" in header


def test_null_handle_is_rejected_by_the_set_op_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_set_op_scratch_bytes(None, 0, 0, 10, 10, ctypes.byref(sz)),
               lib.adlhip_set_op_typed(None, 0, 0, 0, None, None, 10, None, None, 10, 0, None, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


def test_pprims_set_op_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    from oclradixsort_amd.pprims import SET_OPS
    assert SET_OPS == OP_IDS
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    a, b, out = _Buf(np.float32, 100), _Buf(np.float32, 50), _Buf(np.float32, 150)
    va, vb, vout = _Buf(np.int64, 100), _Buf(np.int64, 50), _Buf(np.int64, 150)

    with pytest.raises(AdlHipError, match="needs a device"):
        p.setOp(None, "union", a, b, out, 100, 50)
    for bad in ("xor", "Union", 1, None):
        with pytest.raises(AdlHipError, match="op must be"):
            p.setOp(dev, bad, a, b, out, 100, 50)
    with pytest.raises(AdlHipError, match="both inputs are required"):
        p.setOp(dev, "union", a, None, out, 100, 0)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.setOp(dev, "union", _Buf(bad, 100), _Buf(bad, 50), _Buf(bad, 150), 100, 50)
        with pytest.raises(AdlHipError, match="unsupported values type"):
            p.setOp(dev, "union", a, b, out, 100, 50, valuesA=_Buf(bad, 100), valuesB=_Buf(bad, 50), valuesOut=_Buf(bad, 150))
    with pytest.raises(AdlHipError, match="a is float32, b int32"):
        p.setOp(dev, "union", a, _Buf(np.int32, 50), out, 100, 50)
    for na, nb in ((-1, 50), (101, 50), (100, -1), (100, 51)):
        with pytest.raises(AdlHipError, match="outside"):
            p.setOp(dev, "intersection", a, b, out, na, nb)
    with pytest.raises(AdlHipError, match="fewer than 2\\^32"):
        p.setOp(dev, "union", _Buf(np.uint32, 1 << 31), _Buf(np.uint32, 1 << 31), _Buf(np.uint32, 1 << 32), 1 << 31, 1 << 31)
    # the capacity follows the operation: na for intersection and difference, na + nb for the other two
    for op in ("union", "symmetric_difference"):
        with pytest.raises(AdlHipError, match="out must hold 150"):
            p.setOp(dev, op, a, b, _Buf(np.float32, 149), 100, 50)
    for op in ("intersection", "difference"):
        with pytest.raises(AdlHipError, match="out must hold 100"):
            p.setOp(dev, op, a, b, _Buf(np.float32, 99), 100, 50)
    with pytest.raises(AdlHipError, match="out must hold"):
        p.setOp(dev, "union", a, b, _Buf(np.int32, 150), 100, 50)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.setOp(dev, "union", a, b, None, 100, 50)
    with pytest.raises(AdlHipError, match="valuesA, valuesB and valuesOut go together"):
        p.setOp(dev, "union", a, b, out, 100, 50, valuesA=va, valuesOut=vout)
    with pytest.raises(AdlHipError, match="the values are int64, int32 and int64"):
        p.setOp(dev, "union", a, b, out, 100, 50, valuesA=va, valuesB=_Buf(np.int32, 50), valuesOut=vout)
    with pytest.raises(AdlHipError, match="the values must hold"):
        p.setOp(dev, "union", a, b, out, 100, 50, valuesA=va, valuesB=vb, valuesOut=_Buf(np.int64, 149))
    with pytest.raises(AdlHipError, match="the values must hold"):
        p.setOp(dev, "difference", a, b, out, 100, 50, valuesA=va, valuesB=vb, valuesOut=_Buf(np.int64, 99))
    with pytest.raises(AdlHipError, match="countOut must hold"):
        p.setOp(dev, "union", a, b, out, 100, 50, countOut=_Buf(np.int32, 1))
    with pytest.raises(AdlHipError, match="indexOut must be"):
        p.setOp(dev, "union", a, b, out, 100, 50, indexOut=_Buf(np.uint32, 149))
    with pytest.raises(AdlHipError, match="indexOut must be"):
        p.setOp(dev, "intersection", a, b, out, 100, 50, indexOut=_Buf(np.int64, 100))


def test_torch_sorter_has_the_set_operations():
    from oclradixsort_amd import TorchSorter
    for name, ref in (("intersect", "intersect1d"), ("union", "union1d"), ("difference", "setdiff1d"), ("symmetric_difference", "setxor1d")):
        f = getattr(TorchSorter, name)
        assert callable(f) and ref in f.__doc__
    assert "ONE host read" in TorchSorter.intersect.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a Counter multiset and against thrust's loops
# ---------------------------------------------------------------------------------------------
def _counter(op, a, b):
    ca, cb = collections.Counter(a.tolist()), collections.Counter(b.tolist())
    if op == INTERSECTION:
        return ca & cb
    if op == UNION:
        return ca | cb
    if op == DIFFERENCE:
        return ca - cb
    return (ca - cb) + (cb - ca)


def _thrust_loop(name, order, op, a, b):
    """positions in a || b of the result of thrust's serial set operations (set_operations.h): two pointers; where neither key is in
    front of the other both advance and -- intersection and union -- the element of a is taken"""
    before = (lambda x, y: _typed_less(name, y, x)) if order == DESC else (lambda x, y: _typed_less(name, x, y))
    a, b = a.tolist(), b.tolist()
    i = j = 0
    out = []
    while i < len(a) and j < len(b):
        if before(a[i], b[j]):
            if op != INTERSECTION:
                out.append(i)
            i += 1
        elif before(b[j], a[i]):
            if op in (UNION, SYMMETRIC_DIFFERENCE):
                out.append(len(a) + j)
            j += 1
        else:
            if op in (INTERSECTION, UNION):
                out.append(i)
            i += 1
            j += 1
    if op != INTERSECTION:
        out.extend(range(i, len(a)))
    if op in (UNION, SYMMETRIC_DIFFERENCE):
        out.extend(len(a) + k for k in range(j, len(b)))
    return out


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_setop_oracle_agrees_with_a_counter_and_with_thrusts_loops(name, order):
    rng = np.random.default_rng(29 + BY_NAME[name][1])
    udt = BY_NAME[name][3]
    sp = SPECIALS[np.dtype(udt).itemsize]
    cases = list(_inputs(name, rng))
    cases.append((sp[rng.integers(0, 5, size=90)], sp[rng.integers(0, 5, size=70)]))       # heavy duplication, both ways round
    cases.append((sp[rng.integers(2, 6, size=40)], sp[rng.integers(0, 4, size=95)]))
    cases.append((np.concatenate([sp, sp]), sp))                                            # every key twice against once
    for a, b in cases:
        a, b = sort_bits(a, name, order), sort_bits(b, name, order)
        va = np.arange(a.size, dtype=np.uint64) * np.uint64(3)
        vb = np.arange(b.size, dtype=np.uint64) * np.uint64(5) + np.uint64(1)
        cat, vcat = np.concatenate([a, b]), np.concatenate([va, vb])
        merged = merge_oracle(a, b, name, order)[0].tolist()
        for op in ALL_OPS:
            index, keys, vals, count = setop_oracle(a, b, name, op, order, va, vb)
            assert index.dtype == np.uint32 and keys.dtype == a.dtype and count == index.size == keys.size == vals.size
            assert count <= capacity(op, a.size, b.size)
            assert collections.Counter(keys.tolist()) == _counter(op, a, b), (name, order, OPS[op])
            want = _thrust_loop(name, order, op, a, b)
            assert index.tolist() == want, (name, order, OPS[op], a.size, b.size)
            assert keys.tolist() == [int(cat[i]) for i in want] and vals.tolist() == [int(vcat[i]) for i in want]
            assert is_sorted(keys, name, order)
            # a subsequence of the merge
            it = iter(merged)
            assert all(any(m == i for m in it) for i in want)


def test_oracle_keeps_the_elements_the_contract_names():
    a = np.array([1, 5, 5, 5, 9], np.uint32)       # 5: m = 3
    b = np.array([5, 5, 9, 9, 10], np.uint32)      # 5: n = 2; 9: m = 1, n = 2
    assert setop_oracle(a, b, "u32", INTERSECTION)[0].tolist() == [1, 2, 4]              # the first 2 of A's 5s; A's 9
    assert setop_oracle(a, b, "u32", UNION)[0].tolist() == [0, 1, 2, 3, 4, 8, 9]          # all of A, the last of B's 9s, 10
    assert setop_oracle(a, b, "u32", DIFFERENCE)[0].tolist() == [0, 3]                    # 1, the last of A's 5s
    assert setop_oracle(a, b, "u32", SYMMETRIC_DIFFERENCE)[0].tolist() == [0, 3, 8, 9]
    assert setop_oracle(a[::-1], b[::-1], "u32", UNION, DESC)[1].tolist() == [10, 9, 9, 5, 5, 5, 1]
    # bits decide: -0 is not +0, NaNs are equal by payload
    z = np.array([0x80000000, 0x7fc00001], np.uint32), np.array([0x00000000, 0x7fc00001, 0x7fc00002], np.uint32)
    assert setop_oracle(z[0], z[1], "f32", INTERSECTION)[1].tolist() == [0x7fc00001]
    assert setop_oracle(z[0], z[1], "f32", SYMMETRIC_DIFFERENCE)[1].tolist() == [0x80000000, 0x00000000, 0x7fc00002]
    same = np.full(6, 0x7fc00000, np.uint32)
    for order in (ASC, DESC):
        assert setop_oracle(same, same, "f32", INTERSECTION, order)[0].tolist() == list(range(6))
        assert setop_oracle(same, same, "f32", SYMMETRIC_DIFFERENCE, order)[3] == 0
        assert setop_oracle(same[:4], same, "f32", UNION, order)[0].tolist() == [0, 1, 2, 3, 8, 9]


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def test_setop_demo_host_path_matches_the_oracle(built):
    r = subprocess.run([DEMO, "--host", "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    ok = [ln for ln in lines if ln.startswith("[")]
    per_size = len(ALL_OPS) * 2 * DEMO_PATTERNS * len(DEMO_TYPES)
    assert len(ok) == DEMO_SIZES * per_size, len(ok)
    assert all(ln.startswith("[ OK ] SetOp.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == DEMO_DUMPED * per_size   # the cases with na + nb <= 1000
    seen = set()
    shared = 0
    for ln in dumps:
        head, rest = ln.split(":", 1)
        _, _, oname, kname, vname, dname, na, nb = head.split()
        na, nb, order, op = int(na), int(nb), {"asc": ASC, "desc": DESC}[dname], OP_IDS[oname]
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
        index, keys, vals, count = setop_oracle(a, b, kname, op, order, va, vb)
        assert int(parts[4]) == count, ln[:80]
        assert np.array_equal(_bits(parts[5], kudt), keys) and np.array_equal(_bits(parts[7], np.uint32), index), ln[:80]
        if vname != "none":
            assert np.array_equal(_bits(parts[6], BY_NAME[vname][3]), vals), ln[:80]
        seen.add((oname, kname, vname, dname))
        shared += bool(na and nb and np.intersect1d(a, b).size)
    assert len(seen) == len(ALL_OPS) * 2 * len(DEMO_TYPES)
    assert shared >= len(dumps) // 3, "the demo's cases must make keys of A meet equal keys of B"


def test_facade_exports_the_set_operation(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for k in names:
        for v in names:
            assert re.search(r" W int Tahoe::Pprims::setOp<%s, %s>\(adl::Device const\*, int, adl::Buffer<%s> const&, adl::Buffer<%s> const\*, "
                             r"adl::Buffer<%s> const&, adl::Buffer<%s> const\*, adl::Buffer<%s>&, adl::Buffer<%s>\*, adl::Buffer<unsigned int>\*, "
                             r"int, int, bool\)" % tuple(re.escape(x) for x in (k, v, k, v, k, v, k, v)), out), (k, v)
