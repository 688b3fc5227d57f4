"""Reduce by key: what can be checked without a GPU -- the four symbols and their signatures, the refusals of Pprims.reduceByKey and
Pprims.reduceRuns that need no device, the oracle the GPU tests use (numpy reduceat on the run heads; min / max on the order-preserving
code) against a plain Python loop, and the facade's host path (tests/demo/reduce_demo --host) against numpy -- plus the facade's device
path on the GPU."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "reduce_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
TYPES = {"u32": (np.uint32, np.uint32), "i32": (np.int32, np.uint32), "f32": (np.float32, np.uint32),
         "u64": (np.uint64, np.uint64), "i64": (np.int64, np.uint64), "f64": (np.float64, np.uint64)}
PAIRS = (("u32", "f32"), ("i32", "i64"), ("f32", "i32"), ("u64", "f64"), ("i64", "u32"), ("f64", "u64"))   # the demo's (key, value) types
CASES = 4   # {n, values} pairs of the demo
SUM, MIN, MAX = 0, 1, 2
OPS = {"sum": SUM, "min": MIN, "max": MAX}


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_reduce_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_reduce_runs_scratch_bytes\(adlhip_device\* dev, int key_bytes, int value_type, size_t n, size_t\* work_bytes\);",
                     header)
    assert re.search(r"int adlhip_reduce_runs\(adlhip_device\* dev, int key_bytes, const void\* d_keys_in, int value_type, int op, "
                     r"const void\* d_vals_in, size_t n,\s+void\* d_unique_out, void\* d_reduced_out, uint32_t\* d_counts_out_or_null, "
                     r"uint32_t\* d_offsets_out_or_null,\s+uint32_t\* d_num_runs_out, void\* d_work, size_t work_bytes\);", header)
    assert re.search(r"int adlhip_reduce_by_key_scratch_bytes\(adlhip_device\* dev, int key_type, int value_type, size_t n, size_t\* work_bytes\);",
                     header)
    assert re.search(r"int adlhip_reduce_by_key_typed\(adlhip_device\* dev, int key_type, int order, const void\* d_keys_in, int value_type, "
                     r"int op,\s+const void\* d_vals_in, size_t n, void\* d_unique_out, void\* d_reduced_out,\s+"
                     r"uint32_t\* d_counts_out_or_null, uint32_t\* d_offsets_out_or_null,\s+"
                     r"uint32_t\* d_num_unique_out, void\* d_work, size_t work_bytes\);", header)
    assert re.findall(r"#define (ADLHIP_REDUCE_\w+) (\d)", header) == [("ADLHIP_REDUCE_SUM", "0"), ("ADLHIP_REDUCE_MIN", "1"), ("ADLHIP_REDUCE_MAX", "2")]
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_reduce_runs_scratch_bytes": (I, [VP, I, I, SZ, ctypes.POINTER(SZ)]),
        "adlhip_reduce_runs": (I, [VP, I, VP, I, I, VP, SZ, VP, VP, VP, VP, VP, VP, SZ]),
        "adlhip_reduce_by_key_scratch_bytes": (I, [VP, I, I, SZ, ctypes.POINTER(SZ)]),
        "adlhip_reduce_by_key_typed": (I, [VP, I, I, VP, I, I, VP, SZ, VP, VP, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.reduce_grid"' in header
    # the tile the GPU tests name is the documented one
    kernels = open(os.path.join(ROOT, "oclradixsort_amd", "csrc", "reduce_kernels.hpp")).read()
    assert "kRedTile = 2048 ELEMENTS" in kernels and re.search(r"constexpr int kRedItems = 8;", kernels)


def test_null_handle_is_rejected_by_the_reduce_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_reduce_runs_scratch_bytes(None, 4, 2, 1024, ctypes.byref(sz)),
               lib.adlhip_reduce_by_key_scratch_bytes(None, 2, 2, 1024, ctypes.byref(sz)),
               lib.adlhip_reduce_runs(None, 4, None, 2, 0, None, 1024, None, None, None, None, None, None, 0),
               lib.adlhip_reduce_by_key_typed(None, 2, 0, None, 2, 0, None, 1024, None, None, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.reduceByKey looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_reduce_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    keys, vals = _Buf(np.float32, 100), _Buf(np.int64, 100)
    for fn in (p.reduceByKey, p.reduceRuns):
        with pytest.raises(AdlHipError, match="needs a device"):
            fn(None, keys, vals, 100)
        with pytest.raises(AdlHipError, match="op must be"):
            fn(dev, keys, vals, 100, op="mean")
        for bad in (np.float16, np.uint8, np.int16):
            with pytest.raises(AdlHipError, match="unsupported key type"):
                fn(dev, _Buf(bad, 100), vals, 100)
            with pytest.raises(AdlHipError, match="unsupported value type"):
                fn(dev, keys, _Buf(bad, 100), 100)
        for n in (-1, 101):
            with pytest.raises(AdlHipError, match="outside"):
                fn(dev, keys, vals, n)
        with pytest.raises(AdlHipError, match="outside"):
            fn(dev, keys, _Buf(np.int64, 99), 100)                     # fewer values than keys
        for opt in ("counts", "offsets"):
            with pytest.raises(AdlHipError, match=opt):
                fn(dev, keys, vals, 100, **{opt: _Buf(np.int32, 101)})   # wrong element type
            with pytest.raises(AdlHipError, match=opt):
                fn(dev, keys, vals, 100, **{opt: _Buf(np.uint32, 99)})   # too short
        with pytest.raises(AdlHipError, match="offsets"):
            fn(dev, keys, vals, 100, offsets=_Buf(np.uint32, 100))       # offsets hold n + 1
        with pytest.raises(AdlHipError, match="uniqueOut"):
            fn(dev, keys, vals, 100, uniqueOut=_Buf(np.float64, 100))
        with pytest.raises(AdlHipError, match="uniqueOut"):
            fn(dev, keys, vals, 100, uniqueOut=_Buf(np.float32, 99))
        with pytest.raises(AdlHipError, match="reducedOut"):
            fn(dev, keys, vals, 100, reducedOut=_Buf(np.float32, 100))   # the values' type, not the keys'
        with pytest.raises(AdlHipError, match="reducedOut"):
            fn(dev, keys, vals, 100, reducedOut=_Buf(np.int64, 99))
        with pytest.raises(AdlHipError, match="countOut"):
            fn(dev, keys, vals, 100, countOut=_Buf(np.int32, 1))
        with pytest.raises(AdlHipError, match="countOut"):
            fn(dev, keys, vals, 100, countOut=_Buf(np.uint32, 0))


def test_torch_sorter_has_reduce_by_key_and_reduce_consecutive():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.reduce_by_key) and callable(TorchSorter.reduce_consecutive)
    assert "totalOrder" in TorchSorter.reduce_by_key.__doc__ and "amin" in TorchSorter.reduce_by_key.__doc__
    for name in ("sort", "argsort", "topk", "topk_rows", "unique", "unique_consecutive"):
        assert callable(getattr(TorchSorter, name))


# ---------------------------------------------------------------------------------------------
# the oracle of tests/test_gpu_reduce.py (restated: that file is a GPU module) against a plain loop
# ---------------------------------------------------------------------------------------------
def _encode(bits, name, descending=False):
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


def _decode(code, name):
    w = code.dtype.itemsize
    udt = code.dtype.type
    sign = udt(1 << (8 * w - 1))
    if name[0] == "i":
        return code ^ sign
    if name[0] == "f":
        return np.where(code & sign != 0, code ^ sign, ~code).astype(udt)
    return code.copy()


def _runs_oracle(kbits, vbits, vname, op):
    heads = np.flatnonzero(np.concatenate([[True], kbits[1:] != kbits[:-1]]))
    if op == SUM and vname[0] == "f":
        with np.errstate(all="ignore"):
            red = np.add.reduceat(vbits.view(TYPES[vname][0]), heads).view(vbits.dtype)
    elif op == SUM:
        red = np.add.reduceat(vbits, heads)
    else:
        red = _decode((np.minimum if op == MIN else np.maximum).reduceat(_encode(vbits, vname), heads), vname)
    return kbits[heads], red.astype(vbits.dtype), np.concatenate([heads, [kbits.size]])


def _by_key_oracle(kbits, kname, descending, vbits, vname, op):
    perm = np.argsort(_encode(kbits, kname, descending), kind="stable")
    return _runs_oracle(kbits[perm], vbits[perm], vname, op)


def _total_order_key(bits, name):
    """where a value stands in the ascending order of the typed sorts, stated without the codec: integers by value; floats by sign, then
    magnitude bits (IEEE-754 totalOrder)"""
    w = 4 if name.endswith("32") else 8
    if name[0] == "u":
        return bits
    signed = bits - (1 << (8 * w)) if bits >> (8 * w - 1) else bits
    if name[0] == "i":
        return signed
    mag = bits & ((1 << (8 * w - 1)) - 1)
    return -mag - 1 if bits >> (8 * w - 1) else mag


def _loop_reduce(kbits, vbits, vname, op):
    """one (key, reduced, first position) per run, element by element in Python"""
    w = 4 if vname.endswith("32") else 8
    fmt = {"f32": ("<I", "<f"), "f64": ("<Q", "<d")}.get(vname)
    out = []
    for i, (k, v) in enumerate(zip(kbits.tolist(), vbits.tolist())):
        if not out or out[-1][0] != k:
            out.append([k, v, i])
            continue
        acc = out[-1][1]
        if op == SUM and fmt:
            a = struct.unpack(fmt[1], struct.pack(fmt[0], acc))[0]
            b = struct.unpack(fmt[1], struct.pack(fmt[0], v))[0]
            s = np.float32(a) + np.float32(b) if w == 4 else a + b
            acc = struct.unpack(fmt[0], struct.pack(fmt[1], float(s)))[0]
        elif op == SUM:
            acc = (acc + v) & ((1 << (8 * w)) - 1)
        else:
            kv, ka = _total_order_key(v, vname), _total_order_key(acc, vname)
            if (op == MIN and kv < ka) or (op == MAX and kv > ka):
                acc = v
        out[-1][1] = acc
    return out


SPECIAL32 = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00123, 0xffc00123, 0x7fffffff, 0xffffffff,
             0x00000001, 0x80000001, 0x7f800001, 0xff800001]
SPECIAL64 = [0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000,
             0x7ff8000000000123, 0xfff8000000000123, 0x7fffffffffffffff, 0xffffffffffffffff, 0x0000000000000001, 0x8000000000000001,
             0x7ff0000000000001, 0xfff0000000000001]


@pytest.mark.parametrize("op", ["sum", "min", "max"])
@pytest.mark.parametrize("vname", list(TYPES))
def test_numpy_reduceat_oracle_agrees_with_a_plain_loop(vname, op):
    """np.add.reduceat / np.minimum.reduceat on codes, offsets from the run heads -- the oracle of tests/test_gpu_reduce.py -- against a
    loop over the elements, with NaNs of both signs and payloads, signalling NaNs, +-0, +-inf and the integer extremes among the values"""
    udt = TYPES[vname][1]
    w = np.dtype(udt).itemsize
    rng = np.random.default_rng(5)
    n = 600
    lengths = rng.integers(1, 9, size=n)
    kbits = np.repeat(rng.integers(0, 4, size=n).astype(np.uint32) + np.arange(n, dtype=np.uint32) % 2 * 4, lengths)[:n]   # grouped, values come back
    special = np.array(SPECIAL32 if w == 4 else SPECIAL64, dtype=udt)
    if OPS[op] == SUM and vname[0] == "f":
        vbits = rng.integers(-8, 9, size=n).astype(TYPES[vname][0]).view(udt)      # exact in every association
    else:
        vbits = np.concatenate([special, np.frombuffer(rng.bytes(w * 30), dtype=udt)])[rng.integers(0, special.size + 30, size=n)]
    keys, red, offsets = _runs_oracle(kbits, vbits, vname, OPS[op])
    loop = _loop_reduce(kbits, vbits, vname, OPS[op])
    assert keys.tolist() == [r[0] for r in loop]
    assert offsets[:-1].tolist() == [r[2] for r in loop] and offsets[-1] == n
    assert red.tolist() == [r[1] for r in loop]
    assert len(loop) < n and len(loop) > np.unique(kbits).size     # runs of more than one element; keys that come back
    # a run of one element keeps its bits, whatever they are
    keys, red, _ = _runs_oracle(np.arange(special.size, dtype=np.uint32), special, vname, OPS[op])
    assert np.array_equal(red, special)


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
    assert all(ln.startswith("[ OK ] ReduceByKey.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    for k, v in PAIRS:
        for op in OPS:
            for o in ("ascending", "descending"):
                assert sum(("ReduceByKey.%s.%s %s %s " % (k, v, op, o)) in ln for ln in ok) == CASES, (k, v, op, o)


def test_reduce_demo_host_path_matches_numpy(built):
    lines = _demo_lines(["--host", "--dump"])
    _check_demo(lines)
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == len(PAIRS) * 3 * 2 * 3   # the cases with n <= 1000
    seen = set()
    for ln in dumps:
        head, vals, uout, rout = ln.split("|")
        _, kname, vname, op, order, n = head.split(":")[0].split()
        n = int(n)
        kudt, vudt = TYPES[kname][1], TYPES[vname][1]
        kbits = np.array([int(x, 16) for x in head.split(":")[1].split()], dtype=kudt)
        vbits = np.array([int(x, 16) for x in vals.split()], dtype=vudt)
        got_keys = np.array([int(x, 16) for x in uout.split()], dtype=kudt)
        got_red = np.array([int(x, 16) for x in rout.split()], dtype=vudt)
        assert kbits.size == n and vbits.size == n
        want_keys, want_red, _ = _by_key_oracle(kbits, kname, order == "descending", vbits, vname, OPS[op])
        assert np.array_equal(got_keys, want_keys), (kname, vname, op, order, n)
        assert np.array_equal(got_red, want_red), (kname, vname, op, order, n)
        seen.add((kname, vname, op, order, want_keys.size < n))
    assert len({s[:4] for s in seen}) == len(PAIRS) * 3 * 2
    assert any(s[4] for s in seen), "the demo's keys must repeat"


def test_facade_exports_reduce_by_key(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for k in names:
        for v in names:
            assert re.search(r" W int Tahoe::Pprims::reduceByKey<%s, %s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const&, "
                             r"adl::Buffer<%s>&, adl::Buffer<%s>&, int, int, bool\)" % tuple(re.escape(x) for x in (k, v, k, v, k, v)), out), (k, v)


@pytest.mark.gpu
def test_reduce_demo_device_path(built):
    _check_demo(_demo_lines([]))
