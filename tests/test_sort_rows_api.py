"""Sort along rows: what can be checked without a GPU -- the two symbols and their signatures, the refusals of Pprims.sortRows that need
no device, and the facade's host path (tests/demo/sort_rows_demo --host) against numpy.  The expected order comes from
tests/typed_shapes.py: per row the stable argsort of the keys' ordinals, independent of the codec's formula."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from typed_shapes import ASC, DESC, expected_perm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "sort_rows_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = ("u32", "i32", "f32", "u64", "i64", "f64")
CASES = 7   # {rows, cols, stride} triples of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_sort_rows_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_sort_rows_scratch_bytes\(adlhip_device\* dev, int key_type, size_t rows, size_t cols, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_sort_rows_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, size_t rows, "
                     r"size_t cols,\s+size_t row_stride, void\* d_keys_out_or_null, uint32_t\* d_index_out_or_null,\s+"
                     r"void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["adlhip_sort_rows_scratch_bytes"] == (I, [VP, I, SZ, SZ, ctypes.POINTER(SZ)])
    assert _lib.SIGNATURES["adlhip_sort_rows_typed"] == (I, [VP, I, I, VP, SZ, SZ, SZ, VP, VP, VP, SZ])
    lib = built
    assert lib.adlhip_sort_rows_typed.argtypes == [VP, I, I, VP, SZ, SZ, SZ, VP, VP, VP, SZ]
    assert lib.adlhip_sort_rows_typed.restype is I
    assert lib.adlhip_sort_rows_scratch_bytes.argtypes == [VP, I, SZ, SZ, ctypes.POINTER(SZ)]
    assert '"sort.rows_algo"' in header and '"debug.sort_rows_grid"' in header
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T adlhip_sort_rows_typed" in out and " T adlhip_sort_rows_scratch_bytes" in out


def test_null_handle_is_rejected_by_the_sort_rows_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    assert lib.adlhip_sort_rows_scratch_bytes(None, 2, 8, 1024, ctypes.byref(sz)) == 1   # ADLHIP_FAILURE
    assert b"null device handle" in lib.adlhip_last_error()
    assert lib.adlhip_sort_rows_typed(None, 2, 0, None, 8, 1024, 1024, None, None, None, 0) == 1
    assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.sortRows looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_sort_rows_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    f32 = np.float32
    with pytest.raises(AdlHipError, match="needs a device"):
        p.sortRows(None, _Buf(f32, 400), 4, 100)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.sortRows(dev, _Buf(bad, 400), 4, 100)
    with pytest.raises(AdlHipError, match="rows = -1"):
        p.sortRows(dev, _Buf(f32, 400), -1, 100)
    with pytest.raises(AdlHipError, match="2\\^32"):
        p.sortRows(dev, _Buf(f32, 1 << 33), 1 << 16, 1 << 16)
    with pytest.raises(AdlHipError, match="rowStride"):
        p.sortRows(dev, _Buf(f32, 400), 4, 100, rowStride=99)
    with pytest.raises(AdlHipError, match="keys must hold"):
        p.sortRows(dev, _Buf(f32, 399), 4, 100)                       # (rows - 1) * stride + cols = 400
    with pytest.raises(AdlHipError, match="keys must hold"):
        p.sortRows(dev, _Buf(f32, 414), 4, 100, rowStride=105)        # 3 * 105 + 100 = 415
    with pytest.raises(AdlHipError, match="indexOut"):
        p.sortRows(dev, _Buf(f32, 400), 4, 100, indexOut=_Buf(np.int32, 400))    # wrong element type
    with pytest.raises(AdlHipError, match="indexOut"):
        p.sortRows(dev, _Buf(f32, 400), 4, 100, indexOut=_Buf(np.uint32, 399))   # too short
    with pytest.raises(AdlHipError, match="keysOut"):
        p.sortRows(dev, _Buf(f32, 400), 4, 100, keysOut=_Buf(np.float64, 400))
    with pytest.raises(AdlHipError, match="keysOut"):
        p.sortRows(dev, _Buf(f32, 400), 4, 100, keysOut=_Buf(f32, 399))


def test_torch_sorter_has_sort_rows_and_argsort_rows():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.sort_rows) and callable(TorchSorter.argsort_rows)
    for f in (TorchSorter.sort_rows, TorchSorter.argsort_rows):
        assert "totalOrder" in f.__doc__ and "NaN" in f.__doc__   # where the result differs from torch


def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def check_demo(lines):
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == 12 * CASES, ok
    assert all(ln.startswith("[ OK ] SortRows.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for t in TYPES:
        for o in ("ascending", "descending"):
            assert sum(("SortRows.%s %s " % (t, o)) in ln for ln in ok) == CASES, (t, o)
    # the shapes the demo must cover: both sides of the 4096 keys a workgroup sorts, a padded stride on either side, one row
    shapes = set(tuple(int(x) for x in re.findall(r"rows=(\d+) cols=(\d+) stride=(\d+)", ln)[0]) for ln in ok)
    assert any(c <= 4096 and s > c for _, c, s in shapes) and any(c > 4096 and s > c for _, c, s in shapes)
    assert any(c <= 4096 and s == c for _, c, s in shapes) and any(c > 4096 and s == c for _, c, s in shapes)
    assert any(r == 1 for r, _, _ in shapes)
    return ok


def test_sort_rows_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == 12 * 4   # the cases of at most 2000 keys
    seen = set()
    for ln in dumps:
        head, idx, kout = ln.split("|")
        _, name, order, rows, cols, stride = head.split(":")[0].split()
        rows, cols, stride = int(rows), int(cols), int(stride)
        udt = np.uint32 if name.endswith("32") else np.uint64
        bits = np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=udt)
        got = np.array([int(x) for x in idx.split()], dtype=np.int64).reshape(rows, cols)
        got_keys = np.array([int(x, 16) for x in kout.split()], dtype=udt).reshape(rows, cols)
        assert bits.size == (rows - 1) * stride + cols
        tied = False
        for r in range(rows):
            row = bits[r * stride:r * stride + cols]
            tied |= np.unique(row).size < cols
            want = expected_perm(row, name, DESC if order == "descending" else ASC)
            assert np.array_equal(got[r], want), (name, order, rows, cols, stride, r)
            assert np.array_equal(got_keys[r], row[want]), (name, order, rows, cols, stride, r)
        assert tied, "the demo's keys must tie"
        seen.add((name, order, stride > cols))
    assert len(seen) == 24   # every type and order, with and without padding between the rows


def test_facade_exports_sort_rows(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" W void Tahoe::Pprims::sortRows<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s>&, "
                         r"adl::Buffer<unsigned int>&, int, int, bool, int\)" % ((re.escape(t),) * 3), out), t
        assert re.search(r" W void Tahoe::Pprims::argsortRows<%s>\(adl::Device const\*, adl::Buffer<%s> const&, "
                         r"adl::Buffer<unsigned int>&, int, int, bool, int\)" % ((re.escape(t),) * 2), out), t
