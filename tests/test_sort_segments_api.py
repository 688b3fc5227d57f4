"""Sort within segments: what can be checked without a GPU -- the two symbols and their signatures, the knobs' documentation, the
refusals of the entry points, of Pprims.sortSegments and of TorchSorter.sort_segments that need no device, and the facade's host path
(tests/demo/sort_segments_demo --host) against numpy.  The expected order comes from tests/typed_shapes.py: per segment the stable
argsort of the keys' ordinals, independent of the codec's formula.  The scratch query's formula and the refusals behind a live handle
are checked in test_gpu_sort_segments.py: a handle needs a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from typed_shapes import ASC, DESC, expected_perm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "sort_segments_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = ("u32", "i32", "f32", "u64", "i64", "f64")
CASES = 6   # shapes of the demo


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_sort_segments_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"#define ADLHIP_SEGMENT_INDEX_LOCAL\s+0\b", header) and re.search(r"#define ADLHIP_SEGMENT_INDEX_GLOBAL\s+1\b", header)
    assert re.search(r"int adlhip_sort_segments_scratch_bytes\(adlhip_device\* dev, int key_type, size_t n, size_t num_segments,\s+"
                     r"size_t max_segment,\s+size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_sort_segments_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, size_t n,\s+"
                     r"const uint32_t\* d_offsets,\s+size_t num_segments, size_t max_segment, int index_base,\s+void\* d_keys_out_or_null,\s+"
                     r"uint32_t\* d_index_out_or_null,\s+uint32_t\* d_num_oversized_out_or_null,\s+void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert _lib.SIGNATURES["adlhip_sort_segments_scratch_bytes"] == (I, [VP, I, SZ, SZ, SZ, ctypes.POINTER(SZ)])
    assert _lib.SIGNATURES["adlhip_sort_segments_typed"] == (I, [VP, I, I, VP, SZ, VP, SZ, SZ, I, VP, VP, VP, VP, SZ])
    lib = built
    assert lib.adlhip_sort_segments_typed.argtypes == [VP, I, I, VP, SZ, VP, SZ, SZ, I, VP, VP, VP, VP, SZ]
    assert lib.adlhip_sort_segments_typed.restype is I
    assert lib.adlhip_sort_segments_scratch_bytes.argtypes == [VP, I, SZ, SZ, SZ, ctypes.POINTER(SZ)]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T adlhip_sort_segments_typed" in out and " T adlhip_sort_segments_scratch_bytes" in out


def test_knobs_are_documented_with_their_ranges(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r'"sort\.segments_algo" -1 \[default\] / 0 / 1', header)
    assert re.search(r'"debug\.sort_segments_grid" workgroups .* at most \(0 \[default\]', header)
    handle = open(os.path.join(ROOT, "oclradixsort_amd", "csrc", "handle.hip")).read()
    assert re.search(r'\{"sort\.segments_algo", &adlhip_device::sort_segments_algo, -1, 1,', handle)
    assert re.search(r'\{"debug\.sort_segments_grid", &adlhip_device::sort_segments_grid, 0, kNoMax,', handle)


def test_null_handle_is_rejected_by_the_sort_segments_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    assert lib.adlhip_sort_segments_scratch_bytes(None, 2, 1024, 8, 128, ctypes.byref(sz)) == 1   # ADLHIP_FAILURE
    assert b"null device handle" in lib.adlhip_last_error()
    assert lib.adlhip_sort_segments_typed(None, 2, 0, None, 1024, None, 8, 128, 0, None, None, None, None, 0) == 1
    assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.sortSegments looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_sort_segments_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    f32, u32 = np.float32, np.uint32
    with pytest.raises(AdlHipError, match="needs a device"):
        p.sortSegments(None, _Buf(f32, 400), _Buf(u32, 5), 4)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.sortSegments(dev, _Buf(bad, 400), _Buf(u32, 5), 4)
    with pytest.raises(AdlHipError, match="numSegments = -1"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), -1)
    with pytest.raises(AdlHipError, match="maxSegment = -3"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, maxSegment=-3)
    with pytest.raises(AdlHipError, match="2\\^32"):
        p.sortSegments(dev, _Buf(f32, 1 << 32), _Buf(u32, 5), 4)
    with pytest.raises(AdlHipError, match="offsets"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 4), 4)                     # numSegments + 1 = 5 entries
    with pytest.raises(AdlHipError, match="offsets"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(np.int64, 5), 4)                # wrong element type
    with pytest.raises(AdlHipError, match="indexOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, indexOut=_Buf(np.int32, 400))
    with pytest.raises(AdlHipError, match="indexOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, indexOut=_Buf(u32, 399))
    with pytest.raises(AdlHipError, match="keysOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, keysOut=_Buf(np.float64, 400))
    with pytest.raises(AdlHipError, match="keysOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, keysOut=_Buf(f32, 399))
    with pytest.raises(AdlHipError, match="oversizedOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, oversizedOut=_Buf(u32, 0))
    with pytest.raises(AdlHipError, match="oversizedOut"):
        p.sortSegments(dev, _Buf(f32, 400), _Buf(u32, 5), 4, oversizedOut=_Buf(np.int64, 1))


def test_torch_sorter_sort_segments_refuses_without_a_device():
    """the refusals that come before anything touches the device: the sorter here has none"""
    import torch
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.sort_segments) and callable(TorchSorter.argsort_segments)
    for f in (TorchSorter.sort_segments, TorchSorter.argsort_segments):
        assert "totalOrder" in f.__doc__ and "NaN" in f.__doc__ and "host read" in f.__doc__
    s = object.__new__(TorchSorter)   # no handle is opened; close() is never called
    s.torch_device = torch.device("cuda", 0)
    s.device = None
    offs = torch.tensor([0, 3, 10])
    t = torch.arange(10, dtype=torch.float32)
    with pytest.raises(ValueError, match="tensor is on cpu"):
        s.sort_segments(t, offs)                                                 # a CPU tensor
    with pytest.raises(ValueError, match="tensor is on cpu"):
        s.argsort_segments(t, offs, max_segment=7)
    with pytest.raises(TypeError, match="float16"):
        s.sort_segments(t.to(torch.float16), offs)
    with pytest.raises(ValueError, match="1-D tensors only"):
        s.sort_segments(t.reshape(2, 5), offs)
    with pytest.raises(ValueError, match="end at t.numel\\(\\) = 10"):
        s.sort_segments(t, torch.tensor([0, 3, 9]))                              # the last entry is not t.numel()
    with pytest.raises(ValueError, match="start at 0"):
        s.argsort_segments(t, torch.tensor([1, 3, 10], dtype=torch.int32))
    with pytest.raises(ValueError, match="one entry"):
        s.sort_segments(t, torch.tensor([0]), max_segment=4)                     # no segment for ten elements
    with pytest.raises(TypeError, match="int32 or int64"):
        s.sort_segments(t, torch.tensor([0.0, 10.0]))
    with pytest.raises(ValueError, match="num_segments \\+ 1"):
        s.sort_segments(t, offs.reshape(3, 1))
    with pytest.raises(TypeError, match="offsets must be a torch.Tensor"):
        s.sort_segments(t, [0, 3, 10])
    with pytest.raises(TypeError, match="expected a torch.Tensor"):
        s.sort_segments([1.0, 2.0], offs)


def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def check_demo(lines):
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == 12 * CASES, ok
    assert all(ln.startswith("[ OK ] SortSegments.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for t in TYPES:
        for o in ("ascending", "descending"):
            assert sum(("SortSegments.%s %s " % (t, o)) in ln for ln in ok) == CASES, (t, o)
    # the shapes the demo must cover: a bound the segment kernel serves and none, one segment, more keys than a workgroup sorts, both
    # index bases
    shapes = set(tuple(int(x) for x in re.findall(r"segments=(\d+) n=(\d+) max=(\d+) global=(\d)", ln)[0]) for ln in ok)
    assert any(0 < m <= 4096 for _, _, m, _ in shapes) and any(m == 0 and n > 4096 for _, n, m, _ in shapes)
    assert any(s == 1 for s, _, _, _ in shapes) and set(g for _, _, _, g in shapes) == {0, 1}
    return ok


def test_sort_segments_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == 12 * 4   # the cases of at most 2000 keys
    seen, empties = set(), False
    for ln in dumps:
        head, idx, kout = ln.split("|")
        _, name, order, S, n, glob = head.split(":")[0].split()
        S, n, glob = int(S), int(n), int(glob)
        udt = np.uint32 if name.endswith("32") else np.uint64
        offs, keys = head.split(":")[1].split(";")
        offs = np.array([int(x) for x in offs.split()], dtype=np.int64)
        bits = np.array([int(x, 16) for x in keys.split()], dtype=udt)
        got = np.array([int(x) for x in idx.split()], dtype=np.int64)
        got_keys = np.array([int(x, 16) for x in kout.split()], dtype=udt)
        assert offs.size == S + 1 and offs[0] == 0 and offs[-1] == n and bits.size == n and (np.diff(offs) >= 0).all()
        empties |= bool((np.diff(offs) == 0).any()) and len(set(np.diff(offs).tolist())) > 2   # ragged, with empty segments
        tied = S == 0
        for s in range(S):
            a, b = int(offs[s]), int(offs[s + 1])
            seg = bits[a:b]
            tied |= np.unique(seg).size < seg.size
            want = expected_perm(seg, name, DESC if order == "descending" else ASC)
            assert np.array_equal(got[a:b], want + (a if glob else 0)), (name, order, S, n, s)
            assert np.array_equal(got_keys[a:b], seg[want]), (name, order, S, n, s)
        assert tied or n < 40, "the demo's keys must tie"
        seen.add((name, order, glob))
    assert empties
    assert len(seen) == 24   # every type and order, positions inside the segment and in the whole array


def test_facade_exports_sort_segments(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" W void Tahoe::Pprims::sortSegments<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<unsigned int> const&, "
                         r"adl::Buffer<%s>&, adl::Buffer<unsigned int>&, int, int, int, bool, bool\)" % ((re.escape(t),) * 3), out), t
        assert re.search(r" W void Tahoe::Pprims::argsortSegments<%s>\(adl::Device const\*, adl::Buffer<%s> const&, "
                         r"adl::Buffer<unsigned int> const&, adl::Buffer<unsigned int>&, int, int, int, bool, bool\)" % ((re.escape(t),) * 2), out), t
