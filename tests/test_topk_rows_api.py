"""Row-wise top-k: what can be checked without a GPU -- the two symbols and their signatures, the refusals of Pprims.topkRows that need
no device, and the facade's host path (tests/demo/topk_rows_demo --host) against numpy -- plus the facade's device path on the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "topk_rows_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = ("u32", "i32", "f32", "u64", "i64", "f64")
CASES = 6   # {rows, cols, k, stride} quadruples of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_topk_rows_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_topk_rows_scratch_bytes\(adlhip_device\* dev, int key_type, size_t rows, size_t cols, size_t k, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_topk_rows_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, size_t rows, "
                     r"size_t cols,\s+size_t row_stride, size_t k, void\* d_keys_out_or_null, uint32_t\* d_index_out_or_null,\s+"
                     r"void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["adlhip_topk_rows_scratch_bytes"] == (I, [VP, I, SZ, SZ, SZ, ctypes.POINTER(SZ)])
    assert _lib.SIGNATURES["adlhip_topk_rows_typed"] == (I, [VP, I, I, VP, SZ, SZ, SZ, SZ, VP, VP, VP, SZ])
    lib = built
    assert lib.adlhip_topk_rows_typed.argtypes == [VP, I, I, VP, SZ, SZ, SZ, SZ, VP, VP, VP, SZ]
    assert lib.adlhip_topk_rows_typed.restype is I
    assert lib.adlhip_topk_rows_scratch_bytes.argtypes == [VP, I, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    assert '"topk.rows_algo"' in header and '"debug.topk_rows_grid"' in header


def test_null_handle_is_rejected_by_the_topk_rows_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    assert lib.adlhip_topk_rows_scratch_bytes(None, 2, 8, 1024, 16, ctypes.byref(sz)) == 1   # ADLHIP_FAILURE
    assert b"null device handle" in lib.adlhip_last_error()
    assert lib.adlhip_topk_rows_typed(None, 2, 0, None, 8, 1024, 1024, 16, None, None, None, 0) == 1
    assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.topkRows looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_topk_rows_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    f32 = np.float32
    with pytest.raises(AdlHipError, match="needs a device"):
        p.topkRows(None, _Buf(f32, 400), 4, 100, 10)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.topkRows(dev, _Buf(bad, 400), 4, 100, 10)
    for k in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.topkRows(dev, _Buf(f32, 400), 4, 100, k)
    with pytest.raises(AdlHipError, match="rowStride"):
        p.topkRows(dev, _Buf(f32, 400), 4, 100, 10, rowStride=99)
    with pytest.raises(AdlHipError, match="keys must hold"):
        p.topkRows(dev, _Buf(f32, 399), 4, 100, 10)                       # (rows - 1) * stride + cols = 400
    with pytest.raises(AdlHipError, match="keys must hold"):
        p.topkRows(dev, _Buf(f32, 414), 4, 100, 10, rowStride=105)        # 3 * 105 + 100 = 415
    with pytest.raises(AdlHipError, match="indexOut"):
        p.topkRows(dev, _Buf(f32, 400), 4, 100, 10, indexOut=_Buf(np.int32, 40))    # wrong element type
    with pytest.raises(AdlHipError, match="indexOut"):
        p.topkRows(dev, _Buf(f32, 400), 4, 100, 10, indexOut=_Buf(np.uint32, 39))   # too short
    with pytest.raises(AdlHipError, match="keysOut"):
        p.topkRows(dev, _Buf(f32, 400), 4, 100, 10, keysOut=_Buf(np.float64, 40))
    with pytest.raises(AdlHipError, match="keysOut"):
        p.topkRows(dev, _Buf(f32, 400), 4, 100, 10, keysOut=_Buf(f32, 39))


def test_torch_sorter_has_topk_rows():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.topk_rows)


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
    assert all(ln.startswith("[ OK ] TopKRows.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for t in TYPES:
        for o in ("ascending", "descending"):
            assert sum(("TopKRows.%s %s " % (t, o)) in ln for ln in ok) == CASES, (t, o)
    # the shapes the demo must cover: both sides of the 4096 items a workgroup sorts, k == 1, k == cols, a padded stride
    shapes = set(tuple(int(x) for x in re.findall(r"rows=(\d+) cols=(\d+) stride=(\d+) k=(\d+)", ln)[0]) for ln in ok)
    assert any(c < 4096 for _, c, _, _ in shapes) and any(c > 4096 for _, c, _, _ in shapes)
    assert any(k == 1 for _, _, _, k in shapes) and any(k == c for _, c, _, k in shapes)
    assert any(s > c and c < 4096 for _, c, s, _ in shapes) and any(s > c and c > 4096 for _, c, s, _ in shapes)


def test_topk_rows_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    _check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == 12 * 3   # the cases with cols <= 1000
    seen = set()
    for ln in dumps:
        head, idx, kout = ln.split("|")
        _, name, order, rows, cols, stride, k = head.split(":")[0].split()
        rows, cols, stride, k = int(rows), int(cols), int(stride), int(k)
        udt = np.uint32 if name.endswith("32") else np.uint64
        bits = np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=udt)
        got = np.array([int(x) for x in idx.split()], dtype=np.int64).reshape(rows, k)
        got_keys = np.array([int(x, 16) for x in kout.split()], dtype=udt).reshape(rows, k)
        assert bits.size == (rows - 1) * stride + cols
        for r in range(rows):
            row = bits[r * stride:r * stride + cols]
            assert np.unique(row).size < cols // 4, "the demo's keys must tie"
            want = _expected_perm(row, name, order == "descending")[:k]
            assert np.array_equal(got[r], want), (name, order, rows, cols, stride, k, r)
            assert np.array_equal(got_keys[r], row[want]), (name, order, rows, cols, stride, k, r)
        seen.add((name, order, stride > cols))
    assert len(seen) == 24   # every type and order, with and without padding between the rows


def test_facade_exports_topk_rows(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" T Tahoe::Pprims::topKRows\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s>&, "
                         r"adl::Buffer<unsigned int>&, int, int, int, bool, int\)" % (re.escape(t), re.escape(t)), out), t


@pytest.mark.gpu
def test_topk_rows_demo_device_path(built):
    _check_demo(_demo_lines([]))
