"""Histograms: what can be checked without a GPU -- the three symbols and their signatures, the public macros, the knobs, the refusals
of Pprims.histogramRange / binCount and of the torch front end that need no device, the oracle the GPU tests use
(tests/histogram_oracle.py) against a plain Python loop and against numpy.histogram, and the facade's host path
(tests/demo/histogram_demo --host) against that oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from histogram_oracle import BY_NAME, INT_IDS, SPECIAL_KEYS, TYPE_IDS, bincount_oracle, encode, histogram_range_oracle, sort_edges
from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "histogram_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
DEMO_SIZES, DEMO_RANGE_BINS, DEMO_COUNT_BINS = 4, 4, 3


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_histogram_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_histogram_scratch_bytes\(adlhip_device\* dev, int key_type, size_t n, size_t num_bins, int by_edges, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_histogram_range_typed\(adlhip_device\* dev, int key_type, const void\* d_keys_in, size_t n, "
                     r"const void\* d_edges_in,\s+size_t num_bins, int include_upper, uint32_t\* d_counts_out, void\* d_work, "
                     r"size_t work_bytes\);", header)
    assert re.search(r"int adlhip_bincount_typed\(adlhip_device\* dev, int key_type, const void\* d_keys_in, size_t n, size_t num_bins, "
                     r"uint32_t\* d_counts_out,\s+void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_histogram_scratch_bytes": (I, [VP, I, SZ, SZ, I, ctypes.POINTER(SZ)]),
        "adlhip_histogram_range_typed": (I, [VP, I, VP, SZ, VP, SZ, I, VP, VP, SZ]),
        "adlhip_bincount_typed": (I, [VP, I, VP, SZ, SZ, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name


def test_macros_and_knobs_of_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    from oclradixsort_amd import pprims
    assert re.search(r"#define ADLHIP_HISTOGRAM_MAX_RANGE_BINS 4096\b", header)
    assert pprims.HISTOGRAM_MAX_RANGE_BINS == 4096
    m = re.search(r"#define ADLHIP_HISTOGRAM_TILE (\d+)\b", header)
    assert m and int(m.group(1)) == pprims.HISTOGRAM_TILE
    assert '"debug.histogram_grid"' in header and '"debug.histogram_lds_bins"' in header


def test_null_handle_is_rejected_by_the_histogram_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_histogram_scratch_bytes(None, 1, 1024, 16, 1, ctypes.byref(sz)),
               lib.adlhip_histogram_range_typed(None, 2, None, 1024, None, 16, 0, None, None, 0),
               lib.adlhip_bincount_typed(None, 1, None, 1024, 16, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.histogramRange / binCount look at before they make a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_histograms_refuse_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    keys, edges = _Buf(np.float32, 100), _Buf(np.float32, 17)
    ikeys = _Buf(np.int64, 100)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.histogramRange(None, keys, 100, edges)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.binCount(None, ikeys, 100, 10)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.histogramRange(dev, _Buf(bad, 100), 100, _Buf(bad, 17))
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.binCount(dev, _Buf(bad, 100), 100, 10)
    for bad in (np.float32, np.float64):
        with pytest.raises(AdlHipError, match="integer keys only"):
            p.binCount(dev, _Buf(bad, 100), 100, 10)
    with pytest.raises(AdlHipError, match="edges must be a device Buffer"):
        p.histogramRange(dev, keys, 100, [0.0, 1.0])
    with pytest.raises(AdlHipError, match="edges are"):
        p.histogramRange(dev, keys, 100, _Buf(np.float64, 17))
    with pytest.raises(AdlHipError, match="need 18 edges"):
        p.histogramRange(dev, keys, 100, edges, num_bins=17)
    for n in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.histogramRange(dev, keys, n, edges)
        with pytest.raises(AdlHipError, match="outside"):
            p.binCount(dev, ikeys, n, 10)
    with pytest.raises(AdlHipError, match="num_bins = 0 outside"):
        p.histogramRange(dev, keys, 100, _Buf(np.float32, 1))
    with pytest.raises(AdlHipError, match="num_bins = 4097 outside"):
        p.histogramRange(dev, keys, 100, _Buf(np.float32, 4098))
    for bins in (0, -3, 1 << 31):
        with pytest.raises(AdlHipError, match="outside"):
            p.binCount(dev, ikeys, 100, bins)
    with pytest.raises(AdlHipError, match="countsOut must hold"):
        p.histogramRange(dev, keys, 100, edges, countsOut=_Buf(np.uint32, 15))
    with pytest.raises(AdlHipError, match="countsOut must hold"):
        p.binCount(dev, ikeys, 100, 10, countsOut=_Buf(np.int64, 10))


def test_torch_sorter_has_the_histograms():
    from oclradixsort_amd import TorchSorter
    for name in ("bincount", "histogram", "histc"):
        assert callable(getattr(TorchSorter, name))
    assert "reduce_by_key" in TorchSorter.bincount.__doc__ and "ONE host read" in TorchSorter.bincount.__doc__
    assert "numpy.histogram" in TorchSorter.histogram.__doc__
    doc = TorchSorter.histc.__doc__
    assert "numpy.histogram on those edges EXACTLY" in doc and "torch.histc" in doc and "rounding error" in doc
    assert "truncates the edges" in doc and "empty result" in TorchSorter.bincount.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a plain loop and against numpy
# ---------------------------------------------------------------------------------------------
def _typed_less(name, a, b):
    """a sorts before b, stated per type and independently of encode(): integers by value; floats by sign, then by magnitude bits"""
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


def _loop_range(name, keys, edges, include_upper):
    bins = len(edges) - 1
    counts = [0] * bins
    upper = bins - 1
    for b in range(bins - 1, -1, -1):
        if _typed_less(name, edges[b], edges[bins]):
            upper = b
            break
    for k in keys:
        hit = [b for b in range(bins) if not _typed_less(name, k, edges[b]) and _typed_less(name, k, edges[b + 1])]
        assert len(hit) <= 1
        if hit:
            counts[hit[0]] += 1
        elif include_upper and k == edges[bins]:
            counts[upper] += 1
    return counts


@pytest.mark.parametrize("edge_kind", ["distinct", "repeated", "all_equal", "specials"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_range_oracle_agrees_with_a_plain_loop(name, edge_kind):
    udt = BY_NAME[name][3]
    w = np.dtype(udt).itemsize
    rng = np.random.default_rng(31 + BY_NAME[name][1])
    sp = SPECIAL_KEYS[name]
    rnd = np.frombuffer(rng.bytes(w * 60), dtype=udt)
    if edge_kind == "specials":
        e = sp.copy()
    else:
        e = rnd[:9].copy()
        if edge_kind == "repeated":
            e[[1, 4, 5, 8]] = e[[0, 3, 3, 7]]
        if edge_kind == "all_equal":
            e[:] = e[0]
    e = sort_edges(e, name)
    keys = np.concatenate([sp, rnd, e, sp[::-1]])
    for upper in (False, True):
        got = histogram_range_oracle(keys, name, e, upper)
        assert got.dtype == np.uint32 and got.size == e.size - 1
        assert got.tolist() == _loop_range(name, keys.tolist(), e.tolist(), upper), (name, edge_kind, upper)


@pytest.mark.parametrize("name", INT_IDS)
def test_numpy_bincount_oracle_agrees_with_a_plain_loop(name):
    udt, sdt = BY_NAME[name][3], BY_NAME[name][2]
    rng = np.random.default_rng(5)
    keys = np.concatenate([SPECIAL_KEYS[name], rng.integers(-20, 60, size=300).astype(np.int64).astype(sdt).view(udt)])
    for bins in (1, 2, 37, 60, 100):
        want = [0] * bins
        for v in keys.view(sdt).tolist():
            if 0 <= v < bins:
                want[v] += 1
        got = bincount_oracle(keys, name, bins)
        assert got.dtype == np.uint32 and got.tolist() == want, (name, bins)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
def test_range_oracle_with_the_last_bin_closed_is_numpy_histogram(dtype):
    """NaN-free values, +0 only: numpy compares as floats, the oracle on codes"""
    name = {np.float32: "f32", np.float64: "f64", np.int32: "i32", np.int64: "i64"}[dtype]
    rng = np.random.default_rng(11)
    v = (rng.standard_normal(5000) * 40).astype(dtype)
    v[v == 0] = 0   # no -0
    for edges in (np.linspace(-100, 100, 33).astype(dtype), np.array([-50, -50, 0, 7, 7, 7, 120], dtype=dtype), np.array([3, 3], dtype=dtype),
                  np.array([-1000, 1000], dtype=dtype)):
        v[::50] = edges[rng.integers(0, edges.size, size=v[::50].size)]   # values on the edges, the last one among them
        udt = BY_NAME[name][3]
        got = histogram_range_oracle(v.view(udt), name, edges.view(udt), True)
        assert got.astype(np.int64).tolist() == np.histogram(v, bins=edges)[0].tolist(), (name, edges[:4])


def test_range_oracle_orders_zeros_and_nans():
    f = np.array([0xffc00000, 0xff800000, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000, 0x7f800000, 0x7fc00000], dtype=np.uint32)
    assert (np.diff(encode(f, "f32").astype(np.int64)) > 0).all()
    # edges [-0, +0, +inf]: -0 alone in bin 0; +0 and 1 in bin 1; +inf only when the last bin is closed; the NaNs and the rest nowhere
    e = np.array([0x80000000, 0x00000000, 0x7f800000], dtype=np.uint32)
    assert histogram_range_oracle(f, "f32", e, False).tolist() == [1, 2]
    assert histogram_range_oracle(f, "f32", e, True).tolist() == [1, 3]
    # edges that reach the NaNs count them
    e = np.array([0xffc00000, 0xff800000, 0x7f800000, 0x7fc00000], dtype=np.uint32)
    assert histogram_range_oracle(f, "f32", e, True).tolist() == [1, 5, 2]
    # all edges equal: a key on them counts in the last bin, and only when it is closed
    e = np.array([5, 5, 5, 5], dtype=np.uint32)
    k = np.array([4, 5, 5, 6], dtype=np.uint32)
    assert histogram_range_oracle(k, "u32", e, False).tolist() == [0, 0, 0]
    assert histogram_range_oracle(k, "u32", e, True).tolist() == [0, 0, 2]
    # the last edge repeated: the closed bin is the last one with a lower edge below it
    e = np.array([0, 5, 9, 9], dtype=np.uint32)
    k = np.array([9, 9, 5, 0, 10], dtype=np.uint32)
    assert histogram_range_oracle(k, "u32", e, True).tolist() == [1, 3, 0]


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def check_demo_output(stdout):
    """every line of histogram_demo --dump against the oracle; shared with the GPU test of the facade"""
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == DEMO_SIZES * (DEMO_RANGE_BINS * 2 * len(TYPE_IDS) + DEMO_COUNT_BINS * len(INT_IDS)), len(ok)
    assert all(ln.startswith("[ OK ] Histogram.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    # the cases with n <= 1000 and: at most 64 range bins, at most 1000 bincount bins
    assert len(dumps) == (DEMO_SIZES - 1) * ((DEMO_RANGE_BINS - 1) * 2 * len(TYPE_IDS) + (DEMO_COUNT_BINS - 1) * len(INT_IDS))
    seen = set()
    counted = 0
    for ln in dumps:
        head, rest = ln.split(":", 1)
        words = head.split()
        parts = rest.split("|")
        if words[1] == "range":
            _, _, tname, upper, n, bins = words
            n, bins, udt = int(n), int(bins), BY_NAME[tname][3]
            keys, edges = _bits(parts[0], udt), _bits(parts[1], udt)
            got = np.array([int(x) for x in parts[2].split()], dtype=np.uint32)
            assert keys.size == n and edges.size == bins + 1 and got.size == bins
            assert np.array_equal(got, histogram_range_oracle(keys, tname, edges, upper == "1")), ln[:80]
            seen.add(("range", tname, upper))
        else:
            _, _, tname, n, bins = words
            n, bins, udt = int(n), int(bins), BY_NAME[tname][3]
            keys = _bits(parts[0], udt)
            got = np.array([int(x) for x in parts[1].split()], dtype=np.uint32)
            assert keys.size == n and got.size == bins
            assert np.array_equal(got, bincount_oracle(keys, tname, bins)), ln[:80]
            seen.add(("bincount", tname))
        counted += int(got.sum()) > 0
    assert len(seen) == 2 * len(TYPE_IDS) + len(INT_IDS)
    assert counted > len(dumps) // 2, "the demo's cases must count some keys"


def test_histogram_demo_host_path_matches_the_oracle(built):
    r = subprocess.run([DEMO, "--host", "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    check_demo_output(r.stdout)


def test_facade_exports_the_histograms(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for k in names:
        assert re.search(r" W void Tahoe::Pprims::histogramRange<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const&, "
                         r"adl::Buffer<unsigned int>&, int, int, bool\)" % tuple(re.escape(x) for x in (k, k, k)), out), k
        if k not in ("float", "double"):
            assert re.search(r" W void Tahoe::Pprims::binCount<%s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<unsigned int>&, "
                             r"int, int\)" % tuple(re.escape(x) for x in (k, k)), out), k
