"""Unique / run-length encode: what can be checked without a GPU -- the four symbols and their signatures, the refusals of Pprims.unique
and Pprims.runLengthEncode that need no device, the oracle the GPU tests use (numpy on the encoded ordinal) against the stable argsort's
run heads, and the facade's host path (tests/demo/unique_demo --host) against numpy -- plus the facade's device path on the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "unique_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = ("u32", "i32", "f32", "u64", "i64", "f64")
CASES = 5   # {n, values} pairs of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_unique_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_run_length_encode_scratch_bytes\(adlhip_device\* dev, int key_bytes, size_t n, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_run_length_encode\(adlhip_device\* dev, int key_bytes, const void\* d_keys_in, size_t n,\s+"
                     r"void\* d_unique_out, uint32_t\* d_counts_out_or_null, uint32_t\* d_offsets_out_or_null,\s+"
                     r"uint32_t\* d_num_runs_out, void\* d_work, size_t work_bytes\);", header)
    assert re.search(r"int adlhip_unique_scratch_bytes\(adlhip_device\* dev, int key_type, size_t n, int want_index, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_unique_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, size_t n,\s+"
                     r"void\* d_unique_out, uint32_t\* d_counts_out_or_null, uint32_t\* d_offsets_out_or_null,\s+"
                     r"uint32_t\* d_first_index_out_or_null, uint32_t\* d_inverse_out_or_null,\s+"
                     r"uint32_t\* d_num_unique_out, void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_run_length_encode_scratch_bytes": (I, [VP, I, SZ, ctypes.POINTER(SZ)]),
        "adlhip_run_length_encode": (I, [VP, I, VP, SZ, VP, VP, VP, VP, VP, SZ]),
        "adlhip_unique_scratch_bytes": (I, [VP, I, SZ, I, ctypes.POINTER(SZ)]),
        "adlhip_unique_typed": (I, [VP, I, I, VP, SZ, VP, VP, VP, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"unique.algo"' in header and '"debug.unique_grid"' in header
    # the set of key types and orders is what it was
    assert re.findall(r"#define (ADLHIP_(?:KEY|ORDER)_\w+)", header) == [
        "ADLHIP_KEY_U32", "ADLHIP_KEY_I32", "ADLHIP_KEY_F32", "ADLHIP_KEY_U64", "ADLHIP_KEY_I64", "ADLHIP_KEY_F64",
        "ADLHIP_ORDER_ASCENDING", "ADLHIP_ORDER_DESCENDING"]


def test_null_handle_is_rejected_by_the_unique_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_run_length_encode_scratch_bytes(None, 4, 1024, ctypes.byref(sz)),
               lib.adlhip_unique_scratch_bytes(None, 2, 1024, 1, ctypes.byref(sz)),
               lib.adlhip_run_length_encode(None, 4, None, 1024, None, None, None, None, None, 0),
               lib.adlhip_unique_typed(None, 2, 0, None, 1024, None, None, None, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.unique looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_unique_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    keys = _Buf(np.float32, 100)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.unique(None, keys, 100)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.runLengthEncode(None, keys, 100)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.unique(dev, _Buf(bad, 100), 100)
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.runLengthEncode(dev, _Buf(bad, 100), 100)
    for n in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.unique(dev, keys, n)
        with pytest.raises(AdlHipError, match="outside"):
            p.runLengthEncode(dev, keys, n)
    for opt in ("counts", "offsets", "firstIndex", "inverse"):
        with pytest.raises(AdlHipError, match=opt):
            p.unique(dev, keys, 100, **{opt: _Buf(np.int32, 101)})     # wrong element type
        with pytest.raises(AdlHipError, match=opt):
            p.unique(dev, keys, 100, **{opt: _Buf(np.uint32, 99)})     # too short
    with pytest.raises(AdlHipError, match="offsets"):
        p.unique(dev, keys, 100, offsets=_Buf(np.uint32, 100))         # offsets hold n + 1
    with pytest.raises(AdlHipError, match="offsets"):
        p.runLengthEncode(dev, keys, 100, offsets=_Buf(np.uint32, 100))
    with pytest.raises(AdlHipError, match="counts"):
        p.runLengthEncode(dev, keys, 100, counts=_Buf(np.int64, 100))
    for fn in (p.unique, p.runLengthEncode):
        with pytest.raises(AdlHipError, match="uniqueOut"):
            fn(dev, keys, 100, uniqueOut=_Buf(np.float64, 100))
        with pytest.raises(AdlHipError, match="uniqueOut"):
            fn(dev, keys, 100, uniqueOut=_Buf(np.float32, 99))
        with pytest.raises(AdlHipError, match="countOut"):
            fn(dev, keys, 100, countOut=_Buf(np.int32, 1))
        with pytest.raises(AdlHipError, match="countOut"):
            fn(dev, keys, 100, countOut=_Buf(np.uint32, 0))


def test_torch_sorter_has_unique_and_unique_consecutive():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.unique) and callable(TorchSorter.unique_consecutive)
    for name in ("sort", "argsort", "topk", "topk_rows"):
        assert callable(getattr(TorchSorter, name))


# the order-preserving code of a key (include/adlhip.h, "typed keys"): unsigned ascending order of the code is the order of the keys
def _encode(bits, name, descending):
    w = bits.dtype.itemsize
    udt = bits.dtype.type
    sign = udt(1 << (8 * w - 1))
    ones = udt((1 << (8 * w)) - 1)
    e = bits.copy()
    if name[0] == "i":
        e ^= sign
    if name[0] == "f":
        e ^= np.where(bits & sign != 0, ones, sign).astype(udt)
    return ~e if descending else e


# the expected order, from numpy and independent of the codec's formula: the stable argsort of the sign-magnitude ordinal
def _ordinal_halves(bits, name):
    w = bits.dtype.itemsize
    if name[0] == "u":
        if w == 4:
            return bits.astype(np.int64), np.zeros(bits.size, np.int64)
        return (bits >> np.uint64(32)).astype(np.int64), (bits & np.uint64(0xffffffff)).astype(np.int64)
    s = bits.view(np.int32 if w == 4 else np.int64).astype(np.int64)
    if name[0] == "f":
        mx = np.int64(0x7fffffff if w == 4 else 0x7fffffffffffffff)
        s = np.where(s >= 0, s, -(s & mx) - 1)
    if w == 4:
        return s, np.zeros(bits.size, np.int64)
    return s >> np.int64(32), s & np.int64(0xffffffff)


def _expected_perm(bits, name, descending):
    hi, lo = _ordinal_halves(bits, name)
    if descending:
        hi, lo = -hi, -lo
    return np.lexsort((lo, hi))   # stable; the last key is the primary one


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPES)
def test_numpy_unique_of_the_code_gives_the_run_heads_of_the_stable_argsort(name, descending):
    """np.unique(code, return_index=True) -- the oracle of tests/test_gpu_unique.py -- against the definition in include/adlhip.h: the
    run heads of the stable argsort, with NaNs of both signs and two payloads, +-0, +-inf and the integer extremes among the keys"""
    udt = np.uint32 if name.endswith("32") else np.uint64
    w = np.dtype(udt).itemsize
    rng = np.random.default_rng(5)
    if w == 4:
        sp = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00123, 0xffc00123, 0x7fffffff,
                       0xffffffff, 0x00000001, 0x80000001], dtype=udt)
    else:
        sp = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000,
                       0xfff8000000000000, 0x7ff8000000000123, 0xfff8000000000123, 0x7fffffffffffffff, 0xffffffffffffffff,
                       0x0000000000000001, 0x8000000000000001], dtype=udt)
    pool = np.concatenate([sp, np.frombuffer(rng.bytes(w * 20), dtype=udt)])
    bits = pool[rng.integers(0, pool.size, size=3000)]
    code = _encode(bits, name, descending)
    _, first, inverse, counts = np.unique(code, return_index=True, return_inverse=True, return_counts=True)
    perm = _expected_perm(bits, name, descending)
    s = bits[perm]
    heads = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    assert np.array_equal(first, perm[heads])
    assert np.array_equal(bits[first], s[heads])
    assert np.array_equal(counts, np.diff(np.concatenate([heads, [s.size]])))
    assert np.array_equal(bits[first][inverse.reshape(-1)], bits)


def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def _check_demo(lines):
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == 12 * CASES, ok
    assert all(ln.startswith("[ OK ] Unique.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for t in TYPES:
        for o in ("ascending", "descending"):
            assert sum(("Unique.%s %s " % (t, o)) in ln for ln in ok) == CASES, (t, o)


def test_unique_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    _check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == 12 * 3   # the cases with n <= 1000
    seen = set()
    for ln in dumps:
        head, uout, cout = ln.split("|")
        _, name, order, n = head.split(":")[0].split()
        n = int(n)
        udt = np.uint32 if name.endswith("32") else np.uint64
        bits = np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=udt)
        got_keys = np.array([int(x, 16) for x in uout.split()], dtype=udt)
        got_counts = np.array([int(x) for x in cout.split()], dtype=np.int64)
        assert bits.size == n
        code, counts = np.unique(_encode(bits, name, order == "descending"), return_counts=True)
        want = bits[np.unique(_encode(bits, name, order == "descending"), return_index=True)[1]]
        assert code.size == want.size
        assert np.array_equal(got_keys, want), (name, order, n)
        assert np.array_equal(got_counts, counts), (name, order, n)
        seen.add((name, order, n, want.size < n))
    assert len({s[:2] for s in seen}) == 12
    assert any(s[3] for s in seen), "the demo's keys must repeat"


def test_facade_exports_unique(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" T Tahoe::Pprims::unique\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s>&, "
                         r"adl::Buffer<unsigned int>&, int, bool\)" % (re.escape(t), re.escape(t)), out), t


@pytest.mark.gpu
def test_unique_demo_device_path(built):
    _check_demo(_demo_lines([]))
