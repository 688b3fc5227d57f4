"""Stream compaction: what can be checked without a GPU -- the three symbols and their signatures, the ADLHIP_CMP_* values, the knob,
the refusals of Pprims.compactFlagged and Pprims.compactIf that need no device, the oracle the GPU tests use
(tests/compact_oracle.py) against a plain Python loop, and the facade's host path (tests/demo/compact_demo --host) against that
oracle."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from compact_oracle import BY_NAME, CMP_NAMES, CMPS, EQ, GE, GT, LE, LT, NE, SPECIALS, TYPE_IDS, compact_oracle, encode, mask_from_cmp, mask_from_flags
from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "compact_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
DEMO_SIZES = 4
DEMO_FLAGGED = ("f32", "i64")
DEMO_PATTERNS = 5
DEMO_IF = (("u32", "none"), ("i32", "f64"), ("f32", "i32"), ("f32", "none"), ("u64", "f32"), ("i64", "none"), ("f64", "i64"), ("f64", "none"))


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_compact_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_compact_scratch_bytes\(adlhip_device\* dev, size_t n, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_compact_flagged\(adlhip_device\* dev, int item_bytes, const void\* d_items_in_or_null, "
                     r"const uint8_t\* d_flags_in, size_t n,\s+int partition, void\* d_items_out_or_null, uint32_t\* d_index_out_or_null,\s+"
                     r"uint32_t\* d_num_selected_out, void\* d_work, size_t work_bytes\);", header)
    assert re.search(r"int adlhip_compact_if_typed\(adlhip_device\* dev, int key_type, int cmp, const void\* h_threshold, const void\* d_keys_in,\s+"
                     r"int value_bytes, const void\* d_vals_in_or_null, size_t n, int partition,\s+void\* d_keys_out_or_null, "
                     r"void\* d_vals_out_or_null, uint32_t\* d_index_out_or_null,\s+uint32_t\* d_num_selected_out, void\* d_work, "
                     r"size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_compact_scratch_bytes": (I, [VP, SZ, ctypes.POINTER(SZ)]),
        "adlhip_compact_flagged": (I, [VP, I, VP, VP, SZ, I, VP, VP, VP, VP, SZ]),
        "adlhip_compact_if_typed": (I, [VP, I, I, VP, VP, I, VP, SZ, I, VP, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.compact_grid"' in header
    # the run stage the compaction generalises keeps its entry point
    assert "adlhip_run_length_encode" in _lib.SIGNATURES and "int adlhip_run_length_encode(" in header


def test_cmp_codes_of_the_header_the_binding_and_the_oracle(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    from oclradixsort_amd.pprims import CMP_OPS
    for code, name in CMP_NAMES.items():
        assert re.search(r"#define ADLHIP_CMP_%s %d\b" % (name.upper(), code), header), name
        assert CMP_OPS[name] == code
    assert (LT, LE, GT, GE, EQ, NE) == (0, 1, 2, 3, 4, 5)
    assert [CMP_OPS[s] for s in ("<", "<=", ">", ">=", "==", "!=")] == [0, 1, 2, 3, 4, 5]


def test_null_handle_is_rejected_by_the_compact_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_compact_scratch_bytes(None, 1024, ctypes.byref(sz)),
               lib.adlhip_compact_flagged(None, 4, None, None, 1024, 0, None, None, None, None, 0),
               lib.adlhip_compact_if_typed(None, 2, 0, None, None, 0, None, 1024, 0, None, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


class _Buf:
    """what Pprims.compactFlagged looks at before it makes a native call"""

    def __init__(self, dtype, size):
        self.dtype, self._size = np.dtype(dtype), size

    def getSize(self):
        return self._size


def test_pprims_compact_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    flags, items, keys, vals = _Buf(np.uint8, 100), _Buf(np.float32, 100), _Buf(np.int64, 100), _Buf(np.float32, 100)

    with pytest.raises(AdlHipError, match="needs a device"):
        p.compactFlagged(None, flags, 100, items=items)
    with pytest.raises(AdlHipError, match="needs a device"):
        p.compactIf(None, keys, 100, "lt", 3)
    for bad in (np.uint32, np.int16, np.float64):
        with pytest.raises(AdlHipError, match="one byte per element"):
            p.compactFlagged(dev, _Buf(bad, 100), 100, items=items)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported items type"):
            p.compactFlagged(dev, flags, 100, items=_Buf(bad, 100))
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.compactIf(dev, _Buf(bad, 100), 100, "lt", 3)
        with pytest.raises(AdlHipError, match="unsupported values type"):
            p.compactIf(dev, keys, 100, "lt", 3, values=_Buf(bad, 100))
    for n in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.compactFlagged(dev, flags, n, items=items)
        with pytest.raises(AdlHipError, match="outside"):
            p.compactIf(dev, keys, n, "lt", 3)
    with pytest.raises(AdlHipError, match="outside"):
        p.compactFlagged(dev, flags, 100, items=_Buf(np.float32, 99))
    with pytest.raises(AdlHipError, match="outside"):
        p.compactIf(dev, keys, 100, "lt", 3, values=_Buf(np.float32, 99))
    with pytest.raises(AdlHipError, match="cmp must be"):
        p.compactIf(dev, keys, 100, "less", 3)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.compactFlagged(dev, flags, 100)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.compactFlagged(dev, flags, 100, items=items, itemsOut=False)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.compactIf(dev, keys, 100, "lt", 3, keysOut=False)
    with pytest.raises(AdlHipError, match="itemsOut needs items"):
        p.compactFlagged(dev, flags, 100, itemsOut=_Buf(np.float32, 100), indexOut=True)
    with pytest.raises(AdlHipError, match="itemsOut must hold"):
        p.compactFlagged(dev, flags, 100, items=items, itemsOut=_Buf(np.float32, 99))
    with pytest.raises(AdlHipError, match="itemsOut must hold"):
        p.compactFlagged(dev, flags, 100, items=items, itemsOut=_Buf(np.int32, 100))
    with pytest.raises(AdlHipError, match="keysOut must hold"):
        p.compactIf(dev, keys, 100, "lt", 3, keysOut=_Buf(np.float64, 100))
    with pytest.raises(AdlHipError, match="valuesOut must hold"):
        p.compactIf(dev, keys, 100, "lt", 3, values=vals, valuesOut=_Buf(np.float32, 99))
    with pytest.raises(AdlHipError, match="indexOut must be"):
        p.compactFlagged(dev, flags, 100, items=items, indexOut=_Buf(np.uint32, 99))
    with pytest.raises(AdlHipError, match="countOut must hold"):
        p.compactFlagged(dev, flags, 100, items=items, countOut=_Buf(np.uint64, 1))


def test_torch_sorter_has_the_compactions():
    from oclradixsort_amd import TorchSorter
    for name in ("masked_select", "nonzero", "select_if", "partition"):
        assert callable(getattr(TorchSorter, name))
    doc = TorchSorter.select_if.__doc__
    assert "totalOrder" in doc and "NaN and -0 ONLY" in doc and "bit for bit" in doc
    assert "NO broadcasting" in TorchSorter.masked_select.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a plain loop
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


@pytest.mark.parametrize("cmp", CMPS, ids=[CMP_NAMES[c] for c in CMPS])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_compact_oracle_agrees_with_a_plain_loop(name, cmp):
    """encode(keys) cmp encode(threshold), flatnonzero and the stable concatenation -- against a loop over the elements with the
    order stated per type; +-NaN with payloads, +-0, +-inf, denormals and the integer extremes among the keys and as thresholds"""
    udt = BY_NAME[name][3]
    w = np.dtype(udt).itemsize
    rng = np.random.default_rng(17 + BY_NAME[name][1])
    kbits = np.concatenate([SPECIALS[w], np.frombuffer(rng.bytes(w * 40), dtype=udt), SPECIALS[w][::-1]])
    vals = np.arange(kbits.size, dtype=np.uint64) * np.uint64(3)
    for t in np.concatenate([SPECIALS[w], kbits[30:33]]):
        mask = mask_from_cmp(kbits, name, cmp, t)
        loop = []
        for k in kbits.tolist():
            lt, eq = _typed_less(name, k, int(t)), k == int(t)
            loop.append({LT: lt, LE: lt or eq, GT: not lt and not eq, GE: not lt, EQ: eq, NE: not eq}[cmp])
        assert mask.tolist() == loop, (name, cmp, hex(int(t)))
        for partition in (False, True):
            s, index, (kout, vout) = compact_oracle(mask, partition, [kbits, vals])
            want = [i for i, m in enumerate(loop) if m]
            if partition:
                want += [i for i, m in enumerate(loop) if not m]
            assert s == sum(loop) and index.tolist() == want and index.dtype == np.uint32
            assert kout.tolist() == [int(kbits[i]) for i in want] and vout.tolist() == [int(vals[i]) for i in want]


def test_oracle_flags_orders_and_complements():
    flags = np.array([0, 1, 2, 0, 0x80, 0xff, 0], dtype=np.uint8)
    assert mask_from_flags(flags).tolist() == [False, True, True, False, True, True, False]
    assert mask_from_flags(flags.view(np.bool_)).tolist() == mask_from_flags(flags).tolist()
    s, index, (items,) = compact_oracle(mask_from_flags(flags), True, [np.arange(7, dtype=np.uint32) * 10])
    assert s == 4 and index.tolist() == [1, 2, 4, 5, 0, 3, 6] and items.tolist() == [10, 20, 40, 50, 0, 30, 60]
    s, index, _ = compact_oracle(np.zeros(0, bool), True, [])
    assert s == 0 and index.size == 0
    # totalOrder: -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN; -0 is below +0, a NaN equals itself
    f = np.array([0xffc00000, 0xff800000, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000, 0x7f800000, 0x7fc00000], dtype=np.uint32)
    assert (np.diff(encode(f, "f32").astype(np.int64)) > 0).all()
    assert mask_from_cmp(f, "f32", LT, 0).tolist() == [True] * 4 + [False] * 4
    assert mask_from_cmp(f, "f32", EQ, 0x7fc00000).tolist() == [False] * 7 + [True]
    assert mask_from_cmp(f, "f32", GE, 0x80000000).tolist() == [False] * 3 + [True] * 5
    i = np.array([0x80000000, 0xffffffff, 0, 1, 0x7fffffff], dtype=np.uint32)
    assert mask_from_cmp(i, "i32", LT, 0).tolist() == [True, True, False, False, False]
    assert mask_from_cmp(i, "u32", LT, 0x80000000).tolist() == [False, False, True, True, True]
    # LT / GE and EQ / NE are complements
    for name in TYPE_IDS:
        k = SPECIALS[np.dtype(BY_NAME[name][3]).itemsize]
        for t in k:
            assert (mask_from_cmp(k, name, LT, t) ^ mask_from_cmp(k, name, GE, t)).all()
            assert (mask_from_cmp(k, name, EQ, t) ^ mask_from_cmp(k, name, NE, t)).all()
            assert (mask_from_cmp(k, name, LE, t) ^ mask_from_cmp(k, name, GT, t)).all()
    assert struct.unpack("<I", struct.pack("<f", -0.0))[0] == 0x80000000


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if ln.strip()]


def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def test_compact_demo_host_path_matches_the_oracle(built):
    lines = _demo_lines(["--host", "--dump"])
    ok = [ln for ln in lines if ln.startswith("[")]
    per_size = len(DEMO_FLAGGED) * DEMO_PATTERNS + len(DEMO_IF) * len(CMPS)
    assert len(ok) == DEMO_SIZES * 2 * per_size, len(ok)
    assert all(ln.startswith("[ OK ] Compact.") for ln in ok), [ln for ln in ok if not ln.startswith("[ OK ]")]
    dumps = [ln for ln in lines if ln.startswith("DUMP ")]
    assert len(dumps) == (DEMO_SIZES - 1) * 2 * per_size   # the cases with n <= 1000
    seen = set()
    mid = 0
    for ln in dumps:
        head, rest = ln.split(":", 1)
        words = head.split()
        parts = rest.split("|")
        if words[1] == "flagged":
            _, _, tname, mode, n = words
            n, udt = int(n), BY_NAME[tname][3]
            flags, items, s = _bits(parts[0], np.uint8), _bits(parts[1], udt), int(parts[2])
            got, index = _bits(parts[3], udt), _bits(parts[4], np.uint32)
            assert flags.size == n and items.size == n
            es, eindex, (eitems,) = compact_oracle(mask_from_flags(flags), mode == "partition", [items])
            assert s == es and np.array_equal(index, eindex) and np.array_equal(got, eitems), ln[:80]
            seen.add(("flagged", tname, mode))
            mid += 0 < s < n
        else:
            _, _, kname, vname, cmp, tbits, mode, n = words
            n, kudt = int(n), BY_NAME[kname][3]
            keys, s = _bits(parts[0], kudt), int(parts[2])
            assert keys.size == n
            arrays = [keys]
            if vname != "none":
                arrays.append(_bits(parts[1], BY_NAME[vname][3]))
                assert arrays[1].size == n
            code = {v: k for k, v in CMP_NAMES.items()}[cmp]
            es, eindex, eout = compact_oracle(mask_from_cmp(keys, kname, code, int(tbits, 16)), mode == "partition", arrays)
            assert s == es and np.array_equal(_bits(parts[5], np.uint32), eindex), ln[:80]
            assert np.array_equal(_bits(parts[3], kudt), eout[0]), ln[:80]
            if vname != "none":
                assert np.array_equal(_bits(parts[4], BY_NAME[vname][3]), eout[1]), ln[:80]
            seen.add(("if", kname, vname, cmp, mode))
            mid += 0 < s < n
    assert len(seen) == 2 * (len(DEMO_FLAGGED) + len(DEMO_IF) * len(CMPS))
    assert mid > len(dumps) // 4, "the demo's cases must select some elements and reject some"


def test_facade_exports_the_compactions(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    names = ("int", "float", "long long", "double", "unsigned int", "unsigned long long")
    for k in names:
        assert re.search(r" W int Tahoe::Pprims::compactFlagged<%s>\(adl::Device const\*, adl::Buffer<%s> const&, "
                         r"adl::Buffer<unsigned char> const&, adl::Buffer<%s>&, adl::Buffer<unsigned int>\*, int, bool\)"
                         % tuple(re.escape(x) for x in (k, k, k)), out), k
        for v in names:
            assert re.search(r" W int Tahoe::Pprims::compactIf<%s, %s>\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<%s> const\*, "
                             r"int, %s, adl::Buffer<%s>&, adl::Buffer<%s>\*, adl::Buffer<unsigned int>\*, int, bool\)"
                             % tuple(re.escape(x) for x in (k, v, k, v, k, k, v)), out), (k, v)
