"""Join of sorted sequences and expansion of runs: what can be checked without a GPU -- the four symbols and their signatures, the
knob, the kinds and the work formulas in the header, the refusals that need no device (a null handle; what Pprims.joinSorted and
Pprims.expandRuns refuse themselves), the oracle the GPU tests use (tests/join_oracle.py) against a brute-force double loop over all
(i, j) with equal bits, and the facade's host path (tests/demo/join_demo --host) against that oracle."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from oclradixsort_amd import _lib
from join_oracle import (ANTI, ASC, BY_NAME, DESC, INNER, KIND_IDS, KINDS, LEFT, NONE, SEMI, SPECIALS, TYPE_IDS, expand_oracle, is_sorted,
                         join_oracle, join_total, sort_bits)
from test_merge_api import _Buf, _inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "join_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")
ALL_KINDS = (INNER, LEFT, SEMI, ANTI)


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_join_symbols_are_bound_with_the_declared_signatures(built):
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    assert re.search(r"int adlhip_expand_scratch_bytes\(adlhip_device\* dev, size_t num_runs, size_t cap, size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_expand_runs\(adlhip_device\* dev, const uint32_t\* d_counts_in, size_t num_runs,\s+"
                     r"int value_bytes, const void\* d_vals_in_or_null, size_t cap,\s+"
                     r"uint32_t\* d_run_out_or_null, uint32_t\* d_rank_out_or_null, void\* d_vals_out_or_null,\s+"
                     r"uint64_t\* d_num_out, void\* d_work, size_t work_bytes\);", header)
    assert re.search(r"int adlhip_join_scratch_bytes\(adlhip_device\* dev, int key_type, size_t na, size_t nb, size_t cap, "
                     r"size_t\* work_bytes\);", header)
    assert re.search(r"int adlhip_join_sorted_typed\(adlhip_device\* dev, int key_type, int order, int kind,\s+"
                     r"const void\* d_keys_a, size_t na, const void\* d_keys_b, size_t nb, size_t cap,\s+"
                     r"uint32_t\* d_index_a_out_or_null, uint32_t\* d_index_b_out_or_null,\s+"
                     r"uint64_t\* d_num_out, void\* d_work, size_t work_bytes\);", header)
    I, VP, SZ = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    want = {
        "adlhip_expand_scratch_bytes": (I, [VP, SZ, SZ, ctypes.POINTER(SZ)]),
        "adlhip_expand_runs": (I, [VP, VP, SZ, I, VP, SZ, VP, VP, VP, VP, VP, SZ]),
        "adlhip_join_scratch_bytes": (I, [VP, I, SZ, SZ, SZ, ctypes.POINTER(SZ)]),
        "adlhip_join_sorted_typed": (I, [VP, I, I, I, VP, SZ, VP, SZ, SZ, VP, VP, VP, VP, SZ]),
    }
    lib = built
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        fn = getattr(lib, name)
        assert fn.argtypes == sig[1] and fn.restype is I, name
    assert '"debug.join_grid"' in header
    assert re.search(r"#define ADLHIP_JOIN_TILE 2048\b", header)
    for name, value in (("INNER", 0), ("LEFT", 1), ("SEMI", 2), ("ANTI", 3)):
        assert re.search(r"#define ADLHIP_JOIN_%s\s+%d\b" % (name, value), header)
        assert KIND_IDS[name.lower()] == value
    assert re.search(r"#define ADLHIP_JOIN_NONE\s+0xFFFFFFFFu", header) and NONE == 0xFFFFFFFF
    # the header states the work formulas and what holds for inputs that are not sorted
    assert "(8 x 8 x CUs rounded up to 256) + 2 x (4 x na rounded up to 256) + (4 x (tiles + 1) rounded up to 256)" in header
    assert "(8 x 8 x CUs rounded up to 256) + (4 x num_runs rounded up to 256) + (4 x (tiles + 1) rounded up to 256)" in header
    assert "every written index_a is below na, every written index_b is below nb or is ADLHIP_JOIN_NONE" in header
    assert "na + nb <= 0xFFF00000 and na + cap <= 0xFFF00000" in header


def test_null_handle_is_rejected_by_the_join_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    for rc in (lib.adlhip_expand_scratch_bytes(None, 10, 10, ctypes.byref(sz)),
               lib.adlhip_expand_runs(None, None, 10, 0, None, 0, None, None, None, None, None, 0),
               lib.adlhip_join_scratch_bytes(None, 0, 10, 10, 0, ctypes.byref(sz)),
               lib.adlhip_join_sorted_typed(None, 0, 0, 0, None, 10, None, 10, 0, None, None, None, None, 0)):
        assert rc == 1   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error()


def test_pprims_join_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    from oclradixsort_amd.pprims import JOIN_KINDS
    assert JOIN_KINDS == {"inner": 0, "left": 1, "semi": 2, "anti": 3} == KIND_IDS
    p = Pprims()
    dev = object()   # never dereferenced: every refusal below comes first
    a, b = _Buf(np.float32, 100), _Buf(np.float32, 50)
    ia, ib = _Buf(np.uint32, 70), _Buf(np.uint32, 70)

    with pytest.raises(AdlHipError, match="needs a device"):
        p.joinSorted(None, "inner", a, b, 100, 50)
    for bad in ("outer", "Inner", 1, None):
        with pytest.raises(AdlHipError, match="kind must be"):
            p.joinSorted(dev, bad, a, b, 100, 50)
    with pytest.raises(AdlHipError, match="both inputs are required"):
        p.joinSorted(dev, "inner", a, None, 100, 0)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported key type"):
            p.joinSorted(dev, "inner", _Buf(bad, 100), _Buf(bad, 50), 100, 50)
    with pytest.raises(AdlHipError, match="a is float32, b int32"):
        p.joinSorted(dev, "inner", a, _Buf(np.int32, 50), 100, 50)
    for na, nb in ((-1, 50), (101, 50), (100, -1), (100, 51)):
        with pytest.raises(AdlHipError, match="outside"):
            p.joinSorted(dev, "inner", a, b, na, nb)
    with pytest.raises(AdlHipError, match="na \\+ nb"):
        p.joinSorted(dev, "inner", _Buf(np.uint32, 1 << 31), _Buf(np.uint32, 1 << 31), 1 << 31, 1 << 31)
    with pytest.raises(AdlHipError, match="cap = "):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=0xFFF00000 - 99, indexA=_Buf(np.uint32, 1 << 32))
    with pytest.raises(AdlHipError, match="cap = -1"):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=-1)
    with pytest.raises(AdlHipError, match="cap is 0"):
        p.joinSorted(dev, "inner", a, b, 100, 50, indexA=ia)
    with pytest.raises(AdlHipError, match="cap is 0"):
        p.joinSorted(dev, "left", a, b, 100, 50, cap=0, indexB=True)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=70)
    with pytest.raises(AdlHipError, match="countOut must hold"):
        p.joinSorted(dev, "inner", a, b, 100, 50, countOut=_Buf(np.uint32, 1))     # the count is 64 bits wide
    with pytest.raises(AdlHipError, match="countOut must hold"):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=70, indexA=ia, countOut=_Buf(np.uint64, 0))
    with pytest.raises(AdlHipError, match="indexA must be"):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=71, indexA=ia, indexB=ib)
    with pytest.raises(AdlHipError, match="indexB must be"):
        p.joinSorted(dev, "inner", a, b, 100, 50, cap=70, indexA=ia, indexB=_Buf(np.int64, 70))


def test_pprims_expand_runs_refuses_without_a_native_call():
    from oclradixsort_amd import Pprims
    from oclradixsort_amd._lib import AdlHipError
    p = Pprims()
    dev = object()
    counts, vals, vout = _Buf(np.uint32, 100), _Buf(np.float64, 100), _Buf(np.float64, 70)
    run = _Buf(np.uint32, 70)

    with pytest.raises(AdlHipError, match="needs a device"):
        p.expandRuns(None, counts, 100)
    for bad in (None, _Buf(np.int32, 100), _Buf(np.uint64, 100)):
        with pytest.raises(AdlHipError, match="counts must be a uint32 buffer"):
            p.expandRuns(dev, bad, 100)
    for n in (-1, 101):
        with pytest.raises(AdlHipError, match="outside"):
            p.expandRuns(dev, counts, n)
    with pytest.raises(AdlHipError, match="cap = "):
        p.expandRuns(dev, counts, 100, cap=0xFFF00000 - 99, runOut=_Buf(np.uint32, 1 << 32))
    with pytest.raises(AdlHipError, match="values and valuesOut go together"):
        p.expandRuns(dev, counts, 100, cap=70, values=vals)
    with pytest.raises(AdlHipError, match="values and valuesOut go together"):
        p.expandRuns(dev, counts, 100, cap=70, valuesOut=vout)
    for bad in (np.float16, np.uint8, np.int16):
        with pytest.raises(AdlHipError, match="unsupported values type"):
            p.expandRuns(dev, counts, 100, cap=70, values=_Buf(bad, 100), valuesOut=_Buf(bad, 70))
    with pytest.raises(AdlHipError, match="the values are float64 and int64"):
        p.expandRuns(dev, counts, 100, cap=70, values=vals, valuesOut=_Buf(np.int64, 70))
    with pytest.raises(AdlHipError, match="the values must hold"):
        p.expandRuns(dev, counts, 100, cap=71, values=vals, valuesOut=vout)
    with pytest.raises(AdlHipError, match="the values must hold"):
        p.expandRuns(dev, counts, 100, cap=70, values=_Buf(np.float64, 99), valuesOut=vout)
    with pytest.raises(AdlHipError, match="cap is 0"):
        p.expandRuns(dev, counts, 100, runOut=run)
    with pytest.raises(AdlHipError, match="cap is 0"):
        p.expandRuns(dev, counts, 100, values=vals, valuesOut=vout)
    with pytest.raises(AdlHipError, match="nothing asked"):
        p.expandRuns(dev, counts, 100, cap=70)
    with pytest.raises(AdlHipError, match="countOut must hold"):
        p.expandRuns(dev, counts, 100, cap=70, runOut=run, countOut=_Buf(np.uint32, 2))
    with pytest.raises(AdlHipError, match="runOut must be"):
        p.expandRuns(dev, counts, 100, cap=71, runOut=run)
    with pytest.raises(AdlHipError, match="rankOut must be"):
        p.expandRuns(dev, counts, 100, cap=70, runOut=run, rankOut=_Buf(np.int32, 70))


def test_torch_sorter_has_the_join_and_the_expansion():
    from oclradixsort_amd import TorchSorter
    assert callable(TorchSorter.join) and "ONE host read" in TorchSorter.join.__doc__ and "-1" in TorchSorter.join.__doc__
    assert callable(TorchSorter.repeat_interleave) and "torch.repeat_interleave" in TorchSorter.repeat_interleave.__doc__
    assert "nothing reaches the host" in TorchSorter.repeat_interleave.__doc__


# ---------------------------------------------------------------------------------------------
# the oracle against a double loop
# ---------------------------------------------------------------------------------------------
def _double_loop(kind, a, b):
    """the rows of `kind` by looking at every pair (i, j): equal means equal bits.  b is sorted, so the j of one i ascend"""
    a, b = a.tolist(), b.tolist()
    ra, rb = [], []
    for i, x in enumerate(a):
        js = [j for j, y in enumerate(b) if y == x]
        if kind in (INNER, LEFT) or (kind == SEMI and js):
            for j in (js[:1] if kind == SEMI else js):
                ra.append(i)
                rb.append(j)
        if not js and kind in (LEFT, ANTI):
            ra.append(i)
            rb.append(NONE)
    return ra, rb


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
@pytest.mark.parametrize("name", TYPE_IDS)
def test_numpy_join_oracle_agrees_with_a_double_loop(name, order):
    rng = np.random.default_rng(31 + BY_NAME[name][1])
    udt = BY_NAME[name][3]
    sp = SPECIALS[np.dtype(udt).itemsize]
    cases = list(_inputs(name, rng))
    cases.append((sp[rng.integers(0, 5, size=90)], sp[rng.integers(0, 5, size=70)]))       # heavy duplication, both ways round
    cases.append((sp[rng.integers(2, 6, size=40)], sp[rng.integers(0, 4, size=95)]))
    cases.append((np.concatenate([sp, sp]), sp))                                            # every key twice against once
    for a, b in cases:
        a, b = sort_bits(a, name, order), sort_bits(b, name, order)
        assert is_sorted(a, name, order) and is_sorted(b, name, order)
        for kind in ALL_KINDS:
            ia, ib, total = join_oracle(a, b, name, kind, order)
            assert ia.dtype == np.uint32 and ib.dtype == np.uint32 and total == ia.size == ib.size == join_total(a, b, name, kind, order)
            wa, wb = _double_loop(kind, a, b)
            assert ia.tolist() == wa and ib.tolist() == wb, (name, order, KINDS[kind], a.size, b.size)
            for limit in (0, 1, total // 2, total, total + 5):
                la, lb, lt = join_oracle(a, b, name, kind, order, limit=limit)
                r = min(total, limit)
                assert lt == total and la.tolist() == wa[:r] and lb.tolist() == wb[:r]


def test_oracle_gives_the_rows_the_contract_names():
    a = np.array([1, 5, 5, 9, 12], np.uint32)
    b = np.array([5, 5, 5, 9, 10], np.uint32)
    assert [x.tolist() for x in join_oracle(a, b, "u32", INNER)[:2]] == [[1, 1, 1, 2, 2, 2, 3], [0, 1, 2, 0, 1, 2, 3]]
    assert [x.tolist() for x in join_oracle(a, b, "u32", LEFT)[:2]] == [[0, 1, 1, 1, 2, 2, 2, 3, 4], [NONE, 0, 1, 2, 0, 1, 2, 3, NONE]]
    assert [x.tolist() for x in join_oracle(a, b, "u32", SEMI)[:2]] == [[1, 2, 3], [0, 0, 3]]
    assert [x.tolist() for x in join_oracle(a, b, "u32", ANTI)[:2]] == [[0, 4], [NONE, NONE]]
    assert join_oracle(a[::-1], b[::-1], "u32", INNER, DESC)[1].tolist() == [1, 2, 3, 4, 2, 3, 4]
    # bits decide: -0 is not +0, NaNs are equal by payload
    za, zb = np.array([0x80000000, 0x7fc00001], np.uint32), np.array([0x00000000, 0x7fc00001, 0x7fc00002], np.uint32)
    assert [x.tolist() for x in join_oracle(za, zb, "f32", INNER)[:2]] == [[1], [1]]
    # an empty B: nothing for inner and semi, every element of A for left and anti
    e = b[:0]
    assert join_total(a, e, "u32", INNER) == join_total(a, e, "u32", SEMI) == 0
    assert join_oracle(a, e, "u32", LEFT)[1].tolist() == [NONE] * 5 and join_oracle(a, e, "u32", ANTI)[0].tolist() == [0, 1, 2, 3, 4]
    # the count is exact beyond 2^32, and a limited call costs the limit
    big = np.zeros(65537, np.uint32)
    ia, ib, total = join_oracle(big, big, "u32", INNER, limit=4096)
    assert total == 65537 ** 2 > 1 << 32 and not ia.any() and ib.tolist() == list(range(4096))
    run, rank, vals, total = expand_oracle(np.array([2, 0, 3], np.uint32), np.array([7, 8, 9], np.uint64))
    assert (run.tolist(), rank.tolist(), vals.tolist(), total) == ([0, 0, 2, 2, 2], [0, 1, 0, 1, 2], [7, 7, 9, 9, 9], 5)
    assert expand_oracle(np.full(3, 0x7FFFFFFF, np.uint32)[:0])[3] == 0


# ---------------------------------------------------------------------------------------------
# the facade
# ---------------------------------------------------------------------------------------------
def _bits(text, dtype):
    return np.array([int(x, 16) for x in text.split()], dtype=dtype)


def test_join_demo_host_path_matches_the_oracle(built):
    r = subprocess.run([DEMO, "--host", "--dump"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    ok = [ln for ln in lines if ln.startswith("[")]
    assert len(ok) == 432 + 80 and all(ln.startswith("[ OK ] Join.") or ln.startswith("[ OK ] Expand.") for ln in ok), \
        [ln for ln in ok if not ln.startswith("[ OK ]")]
    joins = [ln for ln in lines if ln.startswith("DUMP join ")]
    assert len(joins) == 3 * 4 * 2 * 2 * 6   # the cases with na + nb <= 600
    seen, matched, limited = set(), 0, 0
    for ln in joins:
        head, rest = ln.split(":", 1)
        _, _, kname_kind, kname, dname, na, nb, cap = head.split()
        na, nb, cap, order, kind = int(na), int(nb), int(cap), {"asc": ASC, "desc": DESC}[dname], KIND_IDS[kname_kind]
        parts = rest.split("|")
        udt = BY_NAME[kname][3]
        a, b = _bits(parts[0], udt), _bits(parts[1], udt)
        assert a.size == na and b.size == nb and is_sorted(a, kname, order) and is_sorted(b, kname, order), ln[:80]
        ia, ib, total = join_oracle(a, b, kname, kind, order, limit=cap)
        assert int(parts[2]) == total, ln[:80]
        assert np.array_equal(_bits(parts[3], np.uint32), ia), ln[:80]
        if kind != SEMI:
            assert np.array_equal(_bits(parts[4], np.uint32), ib), ln[:80]
        seen.add((kname_kind, kname, dname))
        matched += bool(kind == INNER and total)
        limited += bool(0 < cap < total)
    assert len(seen) == 4 * 6 * 2
    # 48 inner joins are dumped with both inputs non-empty, and a quarter of the 192 such cases ask for half of the rows
    assert matched >= 40 and limited >= 24, "the demo's cases must make keys of A meet equal keys of B, and cut rows off at cap"
    expands = [ln for ln in lines if ln.startswith("DUMP expand ")]
    assert len(expands) >= 30
    for ln in expands:
        head, rest = ln.split(":", 1)
        _, _, vname, runs, cap = head.split()
        parts = rest.split("|")
        vudt = BY_NAME[vname][3]
        counts, vals = _bits(parts[0], np.uint32), _bits(parts[1], vudt)
        assert counts.size == int(runs) == vals.size
        run, rank, vout, total = expand_oracle(counts, vals)
        r_ = min(total, int(cap))
        assert int(parts[2]) == total
        assert np.array_equal(_bits(parts[3], np.uint32), run[:r_]) and np.array_equal(_bits(parts[4], np.uint32), rank[:r_])
        assert np.array_equal(_bits(parts[5], vudt), vout[:r_])


def test_facade_exports_the_join_and_the_expansion(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for k in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        e = re.escape(k)
        assert re.search(r" W unsigned long long Tahoe::Pprims::joinSorted<%s>\(adl::Device const\*, int, adl::Buffer<%s> const&, "
                         r"adl::Buffer<%s> const&, adl::Buffer<unsigned int>\*, adl::Buffer<unsigned int>\*, int, int, int, bool\)" % (e, e, e), out), k
        assert re.search(r" W unsigned long long Tahoe::Pprims::expandRuns<%s>\(adl::Device const\*, adl::Buffer<unsigned int> const&, "
                         r"adl::Buffer<%s> const\*, adl::Buffer<unsigned int>\*, adl::Buffer<unsigned int>\*, adl::Buffer<%s>\*, int, int\)"
                         % (e, e, e), out), k
