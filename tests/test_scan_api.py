"""Typed scans: what can be checked without a GPU -- the four symbols and their signatures, the knob, the refusals of Pprims.scanTyped
and Pprims.scanByKey that need no device, the oracle the GPU tests use (tests/scan_oracle.py) against a plain Python loop, and the
facade's host path (tests/demo/scan_demo --host) against that oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from scan_oracle import MAX, MIN, OPS, SPECIALS, SUM, TYPES, identity_bits, loop_scan, scan_oracle

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "scan_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
PAIRS = (("none", "f32"), ("none", "i64"), ("none", "u32"), ("none", "f64"), ("u32", "f32"), ("f32", "i64"), ("u64", "i32"), ("f64", "f64"),
         ("i64", "u64"))   # the demo's (key, value) types
CASES = 4   # sizes of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_scan_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_scan_typed_scratch_bytes\(adlhip_device\* dev, int value_type, size_t n, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_scan_typed\(adlhip_device\* dev, int value_type, int op, int exclusive, const void\* h_init_or_null,\s+"
                     r"const void\* d_vals_in,\s+void\* d_out, size_t n, void\* d_work, size_t work_bytes\);", header)
    assert re.search(r"int adlhip_scan_by_key_scratch_bytes\(adlhip_device\* dev, int key_bytes, int value_type, size_t n, size_t\* work_bytes\);",
                     header)
    assert re.search(r"int adlhip_scan_by_key\(adlhip_device\* dev, int key_bytes, const void\* d_keys_in, int value_type, int op, int exclusive,\s+"
                     r"const void\* h_init_or_null, const void\* d_vals_in, void\* d_out, size_t n, void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_scan_typed_scratch_bytes": (I, [VP, I, SZ, ctypes.POINTER(SZ)]),
        "adlhip_scan_typed": (I, [VP, I, I, I, VP, VP, VP, SZ, VP, SZ]),
        "adlhip_scan_by_key_scratch_bytes": (I, [VP, I, I, SZ, ctypes.POINTER(SZ)]),
        "adlhip_scan_by_key": (I, [VP, I, VP, I, I, I, VP, VP, VP, SZ, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.scan_grid"' in header
    # the existing scan keeps its entry point
    assert "adlhip_exclusive_scan_u32" in _lib.SIGNATURES and "int adlhip_exclusive_scan_u32(" in header
    # the scan stage shares the reduce stage's tile, and says what in-place callers rely on
    kernels = open(os.path.join(ROOT, "oclradixsort_amd", "csrc", "scan_kernels.hpp")).read()
    assert '#include "reduce_kernels.hpp"' in kernels and "out == vals" in kernels


def test_null_handle_is_rejected_by_the_scan_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_scan_typed_scratch_bytes(None, 2, 1024, ctypes.byref(sz)),
               lib.adlhip_scan_by_key_scratch_bytes(None, 4, 2, 1024, ctypes.byref(sz)),
               lib.adlhip_scan_typed(None, 2, 0, 0, None, None, None, 1024, None, 0),
               lib.adlhip_scan_by_key(None, 4, None, 2, 0, 0, None, None, None, 1024, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.scanTyped looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_scan_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    keys, src, dst = _Buf(np.float32, 100), _Buf(np.int64, 100), _Buf(np.int64, 100)

    def typed(device, *, keys=keys, dst=dst, src=src, n=100, **kw):
        return p.scanTyped(device, dst, src, n, **kw)

    def by_key(device, *, keys=keys, dst=dst, src=src, n=100, **kw):
        return p.scanByKey(device, keys, dst, src, n, **kw)

    for fn in (typed, by_key):
        with pytest.raises(AdlHipError, match="needs a device"):
            fn(None)
        with pytest.raises(AdlHipError, match="op must be"):
            fn(dev, op="mean")
        for bad in (np.float16, np.uint8, np.int16):
            with pytest.raises(AdlHipError, match="unsupported value type"):
                fn(dev, src=_Buf(bad, 100), dst=_Buf(bad, 100))
        with pytest.raises(AdlHipError, match="dst must have"):
            fn(dev, dst=_Buf(np.float64, 100))
        for n in (-1, 101):
            with pytest.raises(AdlHipError, match="outside"):
                fn(dev, n=n)
        with pytest.raises(AdlHipError, match="outside"):
            fn(dev, dst=_Buf(np.int64, 99))
        with pytest.raises(AdlHipError, match="outside"):
            fn(dev, src=_Buf(np.int64, 99))
        with pytest.raises(AdlHipError, match="no init"):
            fn(dev, init=3)                                            # inclusive
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            by_key(dev, keys=_Buf(bad, 100))
    with pytest.raises(AdlHipError, match="outside"):
        by_key(dev, keys=_Buf(np.float32, 99))


def test_torch_sorter_has_the_scans():
    from oclradixsort_amd import TorchSorter
    for name in ("cumsum", "cummax", "cummin", "scan_by_key"):
        assert callable(getattr(TorchSorter, name))
    assert "totalOrder" in TorchSorter.cummax.__doc__ and "no indices" in TorchSorter.cummax.__doc__
    assert "totalOrder" in TorchSorter.cummin.__doc__ and "no indices" in TorchSorter.cummin.__doc__
    assert "promotes" in TorchSorter.cumsum.__doc__ and "wrap" in TorchSorter.cumsum.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a plain loop
# ---------------------------------------------------------------------------------------------
def _init_bits(vname, op, rng):
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    if op == SUM and vname[0] == "f":
        return np.array([0.1], dtype=dt).view(udt)[0]
    return np.frombuffer(rng.bytes(np.dtype(udt).itemsize), dtype=udt)[0]


@pytest.mark.parametrize("op", ["sum", "min", "max"])
@pytest.mark.parametrize("vname", list(TYPES))
def test_numpy_scan_oracle_agrees_with_a_plain_loop(vname, op):
    """segment ids, cumsum minus the carried-in prefix, maximum.accumulate on folded codes -- against a loop over the elements, with
    NaNs of both signs and payloads, signalling NaNs, +-0, +-inf and the integer extremes among the values; plain and by key, inclusive
    and exclusive, with and without an init"""
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    w = np.dtype(udt).itemsize
    o = OPS[op]
    rng = np.random.default_rng(5 + TYPES[vname][0])
    n = 600
    lengths = rng.integers(1, 9, size=n)
    kbits = np.repeat(rng.integers(0, 4, size=n).astype(np.uint32) + np.arange(n, dtype=np.uint32) % 2 * 4, lengths)[:n]   # grouped, values come back
    if o == SUM and vname[0] == "f":
        vbits = rng.integers(-8, 9, size=n).astype(dt).view(udt)          # exact in every association
    else:
        pool = np.concatenate([SPECIALS[w], np.frombuffer(rng.bytes(w * 30), dtype=udt)])
        vbits = pool[rng.integers(0, pool.size, size=n)]
        if o == SUM:
            vbits[::3] = udt((1 << (8 * w - 1)) - 1)                      # wraps at once
    init = _init_bits(vname, o, rng)
    for keys in (None, kbits, kbits.astype(np.uint64) << np.uint64(31)):
        assert np.array_equal(scan_oracle(keys, vbits, vname, o), loop_scan(keys, vbits, vname, o))
        assert np.array_equal(scan_oracle(keys, vbits, vname, o, True), loop_scan(keys, vbits, vname, o, True))
        assert np.array_equal(scan_oracle(keys, vbits, vname, o, True, init), loop_scan(keys, vbits, vname, o, True, init))
    heads = np.concatenate([[True], kbits[1:] != kbits[:-1]])
    assert 1 < heads.sum() < n and heads.sum() > np.unique(kbits).size   # runs of more than one element; keys that come back
    # heads get the identity pattern / the init; a segment of one element keeps its bits, whatever they are
    ex = scan_oracle(kbits, vbits, vname, o, True)
    assert (ex[heads] == identity_bits(vname, o)).all()
    assert (scan_oracle(kbits, vbits, vname, o, True, init)[heads] == init).all()
    single = np.arange(SPECIALS[w].size, dtype=np.uint32)
    assert np.array_equal(scan_oracle(single, SPECIALS[w], vname, o), SPECIALS[w])
    for m in (0, 1):
        assert scan_oracle(None, vbits[:m], vname, o).size == m and scan_oracle(kbits[:m], vbits[:m], vname, o, True).size == m


def test_identity_patterns_and_the_issue_table():
    assert identity_bits("i32", MIN) == 0x7fffffff and identity_bits("i32", MAX) == 0x80000000 and identity_bits("i32", SUM) == 0
    assert identity_bits("u64", MIN) == 0xffffffffffffffff and identity_bits("u64", MAX) == 0
    assert identity_bits("f32", MIN) == 0x7fffffff and identity_bits("f32", MAX) == 0xffffffff      # +NaN / -NaN, the ends of totalOrder
    assert identity_bits("f64", MIN) == 0x7fffffffffffffff and identity_bits("f64", MAX) == 0xffffffffffffffff
    a, b = 0x7fc00123, 5
    kbits = np.array([a, a, b, a], dtype=np.uint32)
    v = np.array([10, 20, 30, 40], dtype=np.int32).view(np.uint32)
    imax, imin = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    table = {SUM: ([10, 30, 30, 40], [0, 10, 0, 0]), MIN: ([10, 10, 30, 40], [imax, 10, imax, imax]), MAX: ([10, 20, 30, 40], [imin, 10, imin, imin])}
    for op, (inc, exc) in table.items():
        assert scan_oracle(kbits, v, "i32", op).view(np.int32).tolist() == inc
        assert scan_oracle(kbits, v, "i32", op, True).view(np.int32).tolist() == exc
    # -0, +0, -0 -> -0, +0, +0
    z = np.array([-0.0, 0.0, -0.0], dtype=np.float32).view(np.uint32)
    assert scan_oracle(None, z, "f32", SUM).tolist() == [0x80000000, 0, 0]


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def _check_demo(lines):
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == len(PAIRS) * 3 * 2 * CASES, ok
    assert all(ln.startswith("[ OK ] Scan.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for k, v in PAIRS:
        for op in OPS:
            for mode in ("inclusive", "exclusive"):
                assert sum(("Scan.%s.%s %s %s " % (k, v, op, mode)) in ln for ln in ok) == CASES, (k, v, op, mode)


def test_scan_demo_host_path_matches_the_oracle(built):
    lines = _demo_lines(["--host", "--dump"])
    _check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == len(PAIRS) * 3 * 2 * 3   # the cases with n <= 1000
    seen = set()
    for ln in dumps:
        head, vals, out = ln.split("|")
        _, kname, vname, op, mode, n = head.split(":")[0].split()
        n = int(n)
        vudt = TYPES[vname][2]
        kbits = None if kname == "none" else np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=TYPES[kname][2])
        vbits = np.array([int(x, 16) for x in vals.split()], dtype=vudt)
        got = np.array([int(x, 16) for x in out.split()], dtype=vudt)
        assert vbits.size == n and got.size == n and (kbits is None or kbits.size == n)
        want = scan_oracle(kbits, vbits, vname, OPS[op], mode == "exclusive")
        assert np.array_equal(got, want), (kname, vname, op, mode, n)
        segments = 1 if kbits is None else int((kbits[1:] != kbits[:-1]).sum()) + 1
        seen.add((kname, vname, op, mode, 1 < segments < n, kbits is not None and segments > np.unique(kbits).size))
    assert len({s[:4] for s in seen}) == len(PAIRS) * 3 * 2
    assert any(s[4] for s in seen), "the demo's keys must form runs"
    assert any(s[5] for s in seen), "the demo's keys must come back (A A B A)"


def test_facade_exports_the_scans(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for v in names:
        assert re.search(r" W void Tahoe::Pprims::scanTyped<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s>&, int, int, bool\)"
                         % tuple(re.escape(x) for x in (v, v, v)), out), v
        for k in names:
            assert re.search(r" W void Tahoe::Pprims::scanByKey<%s, %s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const&, "
                             r"adl::Buffer<%s>&, int, int, bool\)" % tuple(re.escape(x) for x in (k, v, k, v, v)), out), (k, v)
