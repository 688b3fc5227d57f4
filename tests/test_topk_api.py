"""Top-k: what can be checked without a GPU -- the two symbols and their signatures, the refusals of Pprims.topk that need no device,
and the facade's host path (tests/demo/topk_demo --host) against numpy -- plus the facade's device path on the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "topk_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = ("u32", "i32", "f32", "u64", "i64", "f64")
CASES = 5   # {n, k} pairs of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_topk_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_topk_scratch_bytes\(adlhip_device\* dev, int key_type, size_t n, size_t k, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_topk_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, size_t n, size_t k,\s+"
                     r"void\* d_keys_out_or_null, uint32_t\* d_index_out_or_null, void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["adlhip_topk_scratch_bytes"] == (I, [VP, I, SZ, SZ, ctypes.POINTER(SZ)])
    assert _lib.SIGNATURES["adlhip_topk_typed"] == (I, [VP, I, I, VP, SZ, SZ, VP, VP, VP, SZ])
    lib = built
    assert lib.adlhip_topk_typed.argtypes == [VP, I, I, VP, SZ, SZ, VP, VP, VP, SZ] and lib.adlhip_topk_typed.restype is I
    assert '"topk.algo"' in header


def test_null_handle_is_rejected_by_the_topk_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    assert lib.adlhip_topk_scratch_bytes(None, 2, 1024, 16, ctypes.byref(sz)) == 1   # ADLHIP_FAILURE
    assert b"null device handle" in lib.adlhip_last_error()
    assert lib.adlhip_topk_typed(None, 2, 0, None, 1024, 16, None, None, None, 0) == 1
    assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.topk looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_topk_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    with pytest.raises(AdlHipError, match="needs a device"):
        p.topk(None, _Buf(np.float32, 100), 100, 10)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.topk(dev, _Buf(bad, 100), 100, 10)
    for k in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.topk(dev, _Buf(np.float32, 100), 100, k)
    with pytest.raises(AdlHipError, match="indexOut"):
        p.topk(dev, _Buf(np.float32, 100), 100, 10, indexOut=_Buf(np.int32, 10))    # wrong element type
    with pytest.raises(AdlHipError, match="indexOut"):
        p.topk(dev, _Buf(np.float32, 100), 100, 10, indexOut=_Buf(np.uint32, 9))    # too short
    with pytest.raises(AdlHipError, match="keysOut"):
        p.topk(dev, _Buf(np.float32, 100), 100, 10, keysOut=_Buf(np.float64, 10))
    with pytest.raises(AdlHipError, match="keysOut"):
        p.topk(dev, _Buf(np.float32, 100), 100, 10, keysOut=_Buf(np.float32, 9))


def test_torch_sorter_has_topk():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.topk)


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


def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def _check_demo(lines):
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == 12 * CASES, ok
    assert all(ln.startswith("[ OK ] TopK.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for t in TYPES:
        for o in ("ascending", "descending"):
            assert sum(("TopK.%s %s " % (t, o)) in ln for ln in ok) == CASES, (t, o)


def test_topk_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    _check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == 12 * 3   # the cases with n = 1000
    seen = set()
    for ln in dumps:
        head, idx, kout = ln.split("|")
        _, name, order, n, k = head.split(":")[0].split()
        n, k = int(n), int(k)
        udt = np.uint32 if name.endswith("32") else np.uint64
        bits = np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=udt)
        got = np.array([int(x) for x in idx.split()], dtype=np.int64)
        got_keys = np.array([int(x, 16) for x in kout.split()], dtype=udt)
        assert bits.size == n and got.size == k and got_keys.size == k
        assert np.unique(bits).size < n // 4, "the demo's keys must tie"
        want = _expected_perm(bits, name, order == "descending")[:k]
        assert np.array_equal(got, want), (name, order, n, k)
        assert np.array_equal(got_keys, bits[want]), (name, order, n, k)
        seen.add((name, order))
    assert len(seen) == 12


def test_facade_exports_topk(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" T Tahoe::Pprims::topK\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s>&, "
                         r"adl::Buffer<unsigned int>&, int, int, bool\)" % (re.escape(t), re.escape(t)), out), t


@pytest.mark.gpu
def test_topk_demo_device_path(built):
    _check_demo(_demo_lines([]))
