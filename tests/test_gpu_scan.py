"""Typed scans on the GPU (include/adlhip.h "typed scans"; oclradixsort_amd/csrc/scan_kernels.hpp; Pprims.scanTyped / scanByKey;
TorchSorter.cumsum / cummax / cummin / scan_by_key).

The oracle is tests/scan_oracle.py (numpy; tests/test_scan_api.py checks it against a plain loop on the CPU).  Everything structural is
compared bit for bit: integer sums, min and max always; float sums on values that are small integers stored as floats, whose sums are
exact in every association.  Float sums of random values are held against the textbook bound of any summation order, and the exclusive
scan against the inclusive one bit for bit.

The memory contract is the one of tests/test_gpu_reduce.py, whose plumbing this file uses: every device buffer carries guard bytes
behind its payload -- keys, values, the output (sized exactly n, prefilled with sentinels) and the work buffer (sized exactly the
reported bytes, contents arbitrary, 0x00 or 0xff) --, the inputs are compared with their originals afterwards, and the handle's device
state is idle after each case.

T below is the tile of the scan stage, 2048 elements whatever the widths (reduce_kernels.hpp: kRedTile); PER = the elements of one
16-byte vector of the narrower array.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

import test_gpu_reduce as R
from oclradixsort_amd import Buffer, DeviceUtils, Pprims, _lib
from scan_oracle import MAX, MIN, SPECIALS, SUM, TYPES, combine, heads_of, identity_bits, scan_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OPS = (SUM, MIN, MAX)
OP_NAMES = {SUM: "sum", MIN: "min", MAX: "max"}
TYPE_IDS = list(TYPES)
T = 2048
N40 = 40 * T + 3
SENTINELS = 64
Guarded, lib_err, values_for, keys_from_lengths, sentinels = R.Guarded, R.lib_err, R.values_for, R.keys_from_lengths, R.sentinels
KEY_UDT = {0: None, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    d.setParam("debug.scan_grid", 0)
    DeviceUtils.deallocate(d)


def scan_bytes(dev, kb, vt, n):
    wb = ctypes.c_size_t()
    lib = _lib.load()
    rc = lib.adlhip_scan_by_key_scratch_bytes(dev._h, kb, vt, n, ctypes.byref(wb)) if kb else lib.adlhip_scan_typed_scratch_bytes(
        dev._h, vt, n, ctypes.byref(wb))
    assert rc == 0, lib_err()
    return wb.value


def host_init(init_bits):
    """(keep-alive array, pointer) of one value in host memory; (None, None) without an init"""
    if init_bits is None:
        return None, None
    a = np.array([init_bits])
    return a, a.ctypes.data_as(ctypes.c_void_p)


def call_scan(dev, kb, kptr, vt, op, exclusive, init_ptr, vptr, optr, n, wptr, wbytes):
    lib = _lib.load()
    if kb:
        return lib.adlhip_scan_by_key(dev._h, kb, kptr, vt, op, exclusive, init_ptr, vptr, optr, n, wptr, wbytes)
    return lib.adlhip_scan_typed(dev._h, vt, op, exclusive, init_ptr, vptr, optr, n, wptr, wbytes)


def run_scan(dev, kbits, vname, vbits, op, exclusive=False, init=None, grid=0, exp="oracle", work=None, fill=None, in_place=False):
    """one call of adlhip_scan_typed (kbits None) or adlhip_scan_by_key with every check of the memory contract.  exp: the expected
    bits, "oracle" for scan_oracle's, None when the caller checks the result.  Returns the output as read back."""
    n = vbits.size
    kb = 0 if kbits is None else kbits.dtype.itemsize
    vt, vudt = TYPES[vname][0], TYPES[vname][2]
    assert vbits.dtype == vudt and (kbits is None or kbits.size == n)
    if isinstance(exp, str):
        exp = scan_oracle(kbits, vbits, vname, op, exclusive, init)
    dev.setParam("debug.scan_grid", grid)
    kin = Guarded(dev, kbits, guard_bytes=SENTINELS * kb, seed=5) if kb else None
    vin = Guarded(dev, vbits, guard_bytes=SENTINELS * vbits.dtype.itemsize, seed=6)
    sent = sentinels(vudt, n, 0x3c3c3c3c3c3c3c3c)
    out = vin if in_place else Guarded(dev, sent, guard_bytes=SENTINELS * vbits.dtype.itemsize, seed=7)
    own = work is None
    w = Guarded(dev, nbytes=scan_bytes(dev, kb, vt, n), seed=8, fill=fill) if own else work
    keep, iptr = host_init(None if init is None else vudt(init))
    what = "keys %s, %s %s of %s, init %r, n %d grid %d%s" % (kbits.dtype if kb else "none", "exclusive" if exclusive else "inclusive",
                                                              OP_NAMES[op], vname, init, n, grid, " in place" if in_place else "")
    try:
        rc = call_scan(dev, kb, kin.ptr() if kb else None, vt, op, 1 if exclusive else 0, iptr, vin.ptr(), out.ptr(), n, w.ptr(), w.nbytes)
        assert rc == 0, what + ": " + lib_err()
        got = out.read(vudt).copy()
        if exp is not None and not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            raise AssertionError("%s: differs at %d of %d places, first at %d: got %#x, expected %#x" % (
                what, bad.size, n, bad[0], int(got[bad[0]]), int(exp[bad[0]])))
        w.check_guard()
        if kb:
            assert np.array_equal(kin.read(kbits.dtype), kbits), what + ": d_keys_in was changed"
        if not in_place:
            assert np.array_equal(vin.read(vbits.dtype), vbits), what + ": d_vals_in was changed"
    finally:
        dev.setParam("debug.scan_grid", 0)
        for b in (kin, vin, None if in_place else out, w if own else None):
            if b is not None:
                b.release()
    return got


def random_lengths(n, rng, hi=40):
    lengths = rng.integers(1, hi, size=n)
    lengths = lengths[:np.searchsorted(np.cumsum(lengths), n)]
    return np.concatenate([lengths, [n - lengths.sum()]])


def init_for(vname, op, rng):
    """an init on which the expected bits are exact: a small integer for float sums, any bits otherwise"""
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    if op == SUM and vname[0] == "f":
        return np.array([3.0], dtype=dt).view(udt)[0]
    return np.frombuffer(rng.bytes(np.dtype(udt).itemsize), dtype=udt)[0]


MODES = ((False, False), (True, False), (True, True))   # (exclusive, with an init)


# ---------------------------------------------------------------------------------------------
# every (key width, value type, op, mode)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", TYPE_IDS)
@pytest.mark.parametrize("kw", [0, 4, 8], ids=["plain", "k32", "k64"])
def test_every_key_width_value_type_op_and_mode(dev, kw, vname):
    n = 3 * T + 5
    rng = np.random.default_rng(100 + kw + TYPES[vname][0])
    kbits = keys_from_lengths(KEY_UDT[kw], random_lengths(n, rng), rng, sort=False) if kw else None
    for op in OPS:
        vbits = values_for(vname, op, n, rng)
        for exclusive, with_init in MODES:
            run_scan(dev, kbits, vname, vbits, op, exclusive, init_for(vname, op, rng) if with_init else None)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# sizes: vector, tile and chunk edges
# ---------------------------------------------------------------------------------------------
_SIZE_COMBOS = [(0, "f32"), (4, "f32"), (8, "i64"), (4, "f64")]
_SIZE_CASES = sorted(set((kw, v, n) for kw, v in _SIZE_COMBOS
                         for p in [16 // min(kw or 16, np.dtype(TYPES[v][2]).itemsize)]
                         for n in (0, 1, 2, p - 1, p, p + 1, T - 1, T, T + 1, 2 * T + 3, N40)))


@pytest.mark.parametrize("kw,vname,n", _SIZE_CASES, ids=["k%d-%s-%d" % (8 * c[0], c[1], c[2]) for c in _SIZE_CASES])
def test_sizes(dev, kw, vname, n):
    rng = np.random.default_rng(7 * n + 1)
    vt, vudt = TYPES[vname][0], TYPES[vname][2]
    if n == 0:
        # nothing is written, NULL arrays are accepted
        out = Guarded(dev, sentinels(vudt, 8, 1), seed=3)
        try:
            for excl in (0, 1):
                assert call_scan(dev, kw, None, vt, SUM, excl, None, None, None, 0, None, 0) == 0, lib_err()
                assert call_scan(dev, kw, out.ptr(), vt, MAX, excl, None, out.ptr(), out.ptr(), 0, out.ptr(), 0) == 0, lib_err()
            assert np.array_equal(out.read(vudt), sentinels(vudt, 8, 1))
        finally:
            out.release()
        assert dev.getParam("debug.idle_dirty") == 0
        return
    kbits = keys_from_lengths(KEY_UDT[kw], random_lengths(n, rng, hi=max(2, min(40, n))), rng, sort=False) if kw else None
    for op in OPS:
        vbits = values_for(vname, op, n, rng)
        for exclusive, with_init in MODES:
            run_scan(dev, kbits, vname, vbits, op, exclusive, init_for(vname, op, rng) if with_init else None)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# run shapes x grids x widths; the plain scan at the same grids
# ---------------------------------------------------------------------------------------------
_WIDTHS = [(4, "f32"), (4, "i64"), (8, "f32"), (8, "f64"), (4, "f64"), (8, "i32")]
_SHAPES = [(s, kw, v) for s in R._run_shapes() for kw, v in _WIDTHS]


@pytest.mark.parametrize("shape,kw,vname", _SHAPES, ids=["%s-k%d-%s" % (s, 8 * kw, v) for s, kw, v in _SHAPES])
def test_run_shapes_grids_and_mixed_widths(dev, shape, kw, vname):
    """"debug.scan_grid" 0 gives one tile per chunk, 1 one chunk, 3 chunks of 14 tiles; exact operators give the same bits under all"""
    lengths = R._run_shapes()[shape]
    assert sum(lengths) == N40
    rng = np.random.default_rng(22)
    kbits = keys_from_lengths(KEY_UDT[kw], lengths, rng)
    for op in OPS:
        vbits = values_for(vname, op, N40, rng)
        init = init_for(vname, op, rng)
        exp = {m: scan_oracle(kbits, vbits, vname, op, m[0], init if m[1] else None) for m in MODES}
        for grid in (0, 1, 3):
            for m in MODES:
                run_scan(dev, kbits, vname, vbits, op, m[0], init if m[1] else None, grid=grid, exp=exp[m])
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("vname", TYPE_IDS)
def test_plain_scan_at_three_grids(dev, vname):
    rng = np.random.default_rng(23)
    for op in OPS:
        vbits = values_for(vname, op, N40, rng)
        init = init_for(vname, op, rng)
        exp = {m: scan_oracle(None, vbits, vname, op, m[0], init if m[1] else None) for m in MODES}
        for grid in (0, 1, 3):
            for m in MODES:
                run_scan(dev, None, vname, vbits, op, m[0], init if m[1] else None, grid=grid, exp=exp[m])
    assert dev.getParam("debug.idle_dirty") == 0


def test_scan_grid_knob(dev):
    assert dev.getParam("debug.scan_grid") == 0
    dev.setParam("debug.scan_grid", 3)
    assert dev.getParam("debug.scan_grid") == 3
    dev.setParam("debug.scan_grid", 0)
    with pytest.raises(Exception):
        dev.setParam("debug.scan_grid", -1)
    assert dev.getParam("debug.scan_grid") == 0
    # larger than the default grid: changes nothing, for float sums of random values too
    rng = np.random.default_rng(3)
    kbits = np.sort(rng.integers(0, 900, size=N40).astype(np.uint32))
    vbits = rng.standard_normal(N40).astype(np.float32).view(np.uint32)
    a = run_scan(dev, kbits, "f32", vbits, SUM, exp=None)
    b = run_scan(dev, kbits, "f32", vbits, SUM, grid=1 << 20, exp=None)
    assert np.array_equal(a, b)
    a = run_scan(dev, None, "f32", vbits, SUM, exp=None)
    b = run_scan(dev, None, "f32", vbits, SUM, grid=1 << 20, exp=None)
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------
# in place
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,vname", [(0, "f32"), (0, "i64"), (4, "f32"), (8, "f64"), (4, "i64"), (8, "i32")])
def test_in_place_gives_the_bits_of_the_out_of_place_call(dev, kw, vname):
    rng = np.random.default_rng(33 + kw)
    kbits = keys_from_lengths(KEY_UDT[kw], random_lengths(N40, rng, hi=3 * T), rng, sort=False) if kw else None
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    for op in OPS:
        # random floats for the float sums: the association must be the same one, too
        vbits = rng.standard_normal(N40).astype(dt).view(udt) if (op == SUM and vname[0] == "f") else values_for(vname, op, N40, rng)
        for grid in (0, 3):
            for exclusive, with_init in MODES:
                init = (np.array([0.1], dtype=dt).view(udt)[0] if vname[0] == "f" else init_for(vname, op, rng)) if with_init else None
                apart = run_scan(dev, kbits, vname, vbits, op, exclusive, init, grid=grid, exp=None)
                run_scan(dev, kbits, vname, vbits, op, exclusive, init, grid=grid, exp=apart, in_place=True)
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# cross-checks against the reduce stage and the u32 scan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,vname", [(4, "i64"), (8, "f32"), (4, "u32")])
def test_inclusive_scan_at_run_tails_equals_reduce_runs(dev, kw, vname):
    rng = np.random.default_rng(41)
    kbits = keys_from_lengths(KEY_UDT[kw], random_lengths(N40, rng, hi=2 * T), rng, sort=False)
    tails = np.flatnonzero(np.concatenate([kbits[1:] != kbits[:-1], [True]]))
    for op in OPS:
        vbits = values_for(vname, op, N40, rng)
        for grid in (0, 3):
            inc = run_scan(dev, kbits, vname, vbits, op, grid=grid)
            _, reduced = R.run_reduce(dev, kbits, vname, vbits, op, grid=grid)
            assert np.array_equal(inc[tails], reduced)
    assert dev.getParam("debug.idle_dirty") == 0


def test_plain_exclusive_u32_sum_equals_the_u32_scan(dev):
    rng = np.random.default_rng(42)
    p = Pprims()
    src = dst = None
    try:
        for n in (1, T + 1, N40, 300_001):
            vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
            src, dst = Buffer(dev, n, np.uint32), Buffer(dev, n, np.uint32)
            src.write(vals)
            p.scan(dev, dst, src, n)
            old = dst.toHost()
            assert np.array_equal(run_scan(dev, None, "u32", vals, SUM, True), old)
            src.release()
            dst.release()
            src = dst = None
    finally:
        for b in (src, dst):
            if b is not None:
                b.release()
        p.close()
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# float sums of random values: exclusive against inclusive, the bound of any order, determinism
# ---------------------------------------------------------------------------------------------
def _float_case(vname, rng, n):
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    fixed = np.concatenate([rng.integers(1, 6, size=500), [3 * T + 7, T, 9 * T + 1, 1, 1]])
    mid = rng.integers(50, 400, size=(n - int(fixed.sum()) - 1) // 400)
    rest = n - int(fixed.sum()) - int(mid.sum())
    assert rest > 0
    lengths = np.concatenate([fixed, mid, [5000] * (rest // 5000), [rest % 5000] if rest % 5000 else []]).astype(np.int64)
    lengths = lengths[rng.permutation(lengths.size)]
    assert lengths.sum() == n and lengths.min() == 1 and lengths.max() == 9 * T + 1 and lengths.size < 1000
    kbits = keys_from_lengths(np.uint64, lengths, rng, sort=False)
    vals = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, size=n))).astype(dt)
    return kbits, vals, np.ascontiguousarray(vals).view(udt)


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_exclusive_float_sums_are_a_function_of_the_inclusive_ones(dev, vname):
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    rng = np.random.default_rng(55)
    kbits, _, vbits = _float_case(vname, rng, N40)
    init = np.array([0.1], dtype=dt).view(udt)[0]
    for keys in (kbits, None):
        heads = heads_of(keys, N40)
        for grid in (0, 3):
            inc = run_scan(dev, keys, vname, vbits, SUM, grid=grid, exp=None)
            prev = np.concatenate([inc[:1], inc[:-1]])
            want = np.where(heads, udt(0), prev)                                   # inc[i - 1] bit for bit, zero bits at heads
            run_scan(dev, keys, vname, vbits, SUM, True, grid=grid, exp=want)
            want = np.where(heads, init, combine(np.full(N40, init, dtype=udt), prev, vname, SUM))   # init + inc[i - 1] in the value type
            run_scan(dev, keys, vname, vbits, SUM, True, init, grid=grid, exp=want)
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_sums_of_random_values_within_the_bound_of_any_order_and_deterministic(dev, vname):
    """Every prefix s_i of m elements: |s^ - s| <= gamma_(m-1) sum|x| + u |s|, gamma_k = k u / (1 - k u): the bound of ANY summation order
    of m numbers (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), plus the rounding of the exact sum itself.  s:
    float64 numpy per segment (f32), math.fsum on the sampled prefixes (f64)."""
    n = 64 * T + 1
    dt = TYPES[vname][1]
    u = 2.0 ** -24 if vname == "f32" else 2.0 ** -53
    rng = np.random.default_rng(77)
    kbits, vals, vbits = _float_case(vname, rng, n)
    x = vals.astype(np.float64)
    for keys, samples in ((kbits, 2000), (None, 2000 if vname == "f32" else 150)):
        seen = [run_scan(dev, keys, vname, vbits, SUM, exp=None, fill=fill) for fill in (None, 0x00, 0xff, None)]
        for g in seen[1:]:
            assert np.array_equal(g, seen[0]), "the same call gave other bits"
        got = seen[0].view(dt).astype(np.float64)
        heads = np.flatnonzero(heads_of(keys, n))
        ends = np.concatenate([heads[1:], [n]])
        tails = ends - 1                                                       # every segment's last element, always sampled
        assert tails.size <= samples
        pos = np.unique(np.concatenate([tails, rng.integers(0, n, size=samples - tails.size)]))
        seg = np.searchsorted(heads, pos, side="right") - 1
        worst = 0.0
        for i, s0 in zip(pos.tolist(), heads[seg].tolist()):
            part = x[s0:i + 1]
            m = part.size
            s = math.fsum(part.tolist()) if vname == "f64" else float(part.sum())
            bound = ((m - 1) * u / (1 - (m - 1) * u)) * float(np.abs(part).sum()) + u * abs(s)
            err = abs(float(got[i]) - s)
            worst = max(worst, err / bound if bound else (0.0 if err == 0 else np.inf))
            assert err <= bound, "prefix of %d elements at %d: |%r - %r| = %g > %g" % (m, i, got[i], s, err, bound)
        print("%s %s: largest error / bound over %d prefixes: %.3f" % (vname, "by key" if keys is not None else "plain", pos.size, worst))
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# propagation and special bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vname", ["f32", "f64"])
def test_float_propagation(dev, vname):
    """NaN and the infinities spread to the rest of their segment and not into the next; -0 stays -0; the values are such that every
    association gives the sequential result (numpy's cumsum per segment), but for a NaN's payload"""
    dt, udt = TYPES[vname][1], TYPES[vname][2]
    nan, inf, nz = np.nan, np.inf, -0.0
    runs = [[1.0, 2.0, nan, 3.0] + [1.0] * 300, [nan] + [2.0] * (T + 3), [inf, 1.0, -inf] + [0.5] * 70, [1.0] * (2 * T) + [-inf, 4.0, inf],
            [inf, 1.0, inf] + [-3.0] * 40, [-inf] + [7.0] * (T - 1), [nz] * 2, [nz] * (3 * T + 1), [nz], [nz, 0.0, nz], [1.0, -1.0], [nan, nan],
            [2.0] * 5]
    vals = np.concatenate([np.array(r, dtype=dt) for r in runs])
    kbits = np.repeat(np.arange(len(runs), dtype=np.uint32)[::-1].copy(), [len(r) for r in runs])
    vbits = np.ascontiguousarray(vals).view(udt)
    with np.errstate(all="ignore"):
        want = np.concatenate([np.cumsum(np.array(r, dtype=dt), dtype=dt) for r in runs])
    assert np.isnan(want[2:304]).all() and not np.isnan(want[:2]).any() and want[-1] == 10.0
    for grid in (0, 1, 3):
        got = run_scan(dev, kbits, vname, vbits, SUM, grid=grid, exp=None).view(dt)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
        for op in (MIN, MAX):
            run_scan(dev, kbits, vname, vbits, op, grid=grid)       # the totalOrder oracle
            run_scan(dev, kbits, vname, vbits, op, True, grid=grid)
    # -0, +0, -0 -> -0, +0, +0, plain and as a segment
    z = np.array([nz, 0.0, nz], dtype=dt).view(udt)
    sign = udt(1 << (8 * z.dtype.itemsize - 1))
    assert run_scan(dev, None, vname, z, SUM, exp=None).tolist() == [sign, 0, 0]
    at = sum(len(r) for r in runs[:9])
    assert run_scan(dev, kbits, vname, vbits, SUM, exp=None)[at:at + 3].tolist() == [sign, 0, 0]
    # what totalOrder means here: NaN with the sign bit clear is the largest, -0 is below +0
    hi = scan_oracle(kbits, vbits, vname, MAX).view(dt)
    assert not np.isnan(hi[:2]).any() and np.isnan(hi[2:304]).all()
    lo = scan_oracle(None, z, vname, MIN)
    assert lo.tolist() == [sign, sign, sign] and scan_oracle(None, z, vname, MAX).tolist() == [sign, 0, 0]
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.mark.parametrize("vname", TYPE_IDS)
def test_single_element_segments_return_the_element_bit_for_bit(dev, vname):
    n = 3 * T + 5
    sp = SPECIALS[np.dtype(TYPES[vname][2]).itemsize]
    vbits = np.ascontiguousarray(np.tile(sp, n // sp.size + 1)[:n])
    kbits = np.arange(n, dtype=np.uint32) * np.uint32(7)
    for op in OPS:
        for grid in (0, 2):
            run_scan(dev, kbits, vname, vbits, op, grid=grid, exp=vbits)
            run_scan(dev, kbits.astype(np.uint64), vname, vbits, op, True, grid=grid, exp=np.full(n, identity_bits(vname, op)))
        run_scan(dev, None, vname, vbits[5:6].copy(), op, exp=vbits[5:6])
    assert dev.getParam("debug.idle_dirty") == 0


def test_grouped_but_unsorted_keys(dev):
    """A A B A: three segments; the expected arrays are written out"""
    a, b = 0x7fc00123, 5
    v = np.array([10, 20, 30, 40], dtype=np.int32).view(np.uint32)
    imax, imin = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    table = {SUM: ([10, 30, 30, 40], [0, 10, 0, 0]), MIN: ([10, 10, 30, 40], [imax, 10, imax, imax]), MAX: ([10, 20, 30, 40], [imin, 10, imin, imin])}
    for kudt in (np.uint32, np.uint64):
        kbits = np.array([a, a, b, a], dtype=kudt)
        for op, (inc, exc) in table.items():
            run_scan(dev, kbits, "i32", v, op, exp=np.array(inc, np.int32).view(np.uint32))
            run_scan(dev, kbits, "i32", v, op, True, exp=np.array(exc, np.int32).view(np.uint32))
    # longer: values come back, segments across tiles
    rng = np.random.default_rng(44)
    pool = np.concatenate([np.frombuffer(rng.bytes(8 * 5), dtype=np.uint64), SPECIALS[8][:6]])
    lengths = rng.integers(1, 40, size=900)
    lengths[::97] = T + 1
    picks = rng.integers(0, pool.size, size=lengths.size)
    picks[1:][picks[1:] == picks[:-1]] += 1          # adjacent runs differ
    kbits = np.repeat(pool[picks % pool.size], lengths)
    assert int((kbits[1:] != kbits[:-1]).sum()) + 1 > np.unique(kbits).size, "values must come back"
    vals = rng.integers(-1000, 1000, size=kbits.size).astype(np.int64)
    want, acc = [], 0
    for i, (k, x) in enumerate(zip(kbits.tolist(), vals.tolist())):
        acc = x if i == 0 or k != kbits[i - 1] else acc + x
        want.append(acc)
    for grid in (0, 2):
        run_scan(dev, kbits, "i64", vals.view(np.uint64), SUM, grid=grid, exp=np.array(want, np.int64).view(np.uint64))
    assert dev.getParam("debug.idle_dirty") == 0


# ---------------------------------------------------------------------------------------------
# the work buffer
# ---------------------------------------------------------------------------------------------
def test_scratch_bytes_follow_the_documented_formula(dev):
    """include/adlhip.h: W_scan = 16 CUs + 16 CUs + 32 CUs + 32 CUs + 256, every part rounded up to 256 bytes"""
    cus = DeviceUtils.getNCUs(dev)

    def up(x):
        return (x + 255) // 256 * 256

    for vname in ("i32", "f64"):
        for n in (1, 4097, 100_003, (4 << 20) + 3):
            w_scan = 2 * up(16 * cus) + 2 * up(32 * cus) + 256
            assert scan_bytes(dev, 0, TYPES[vname][0], n) == w_scan
            assert scan_bytes(dev, 4, TYPES[vname][0], n) == w_scan and scan_bytes(dev, 8, TYPES[vname][0], n) == w_scan


def test_scratch_suffices_for_smaller_inputs_and_one_byte_short_is_refused(dev):
    n = 100_003
    rng = np.random.default_rng(8)
    for kw, vname in ((4, "f64"), (8, "i32"), (0, "f32")):
        vt = TYPES[vname][0]
        total = scan_bytes(dev, kw, vt, n)
        assert all(scan_bytes(dev, kw, vt, m) <= total for m in (1, 2049, 50_000))
        w = Guarded(dev, nbytes=total, seed=9)      # one buffer of the size reported for n serves the smaller inputs
        try:
            for m in (1, 2049, 50_000):
                kbits = keys_from_lengths(KEY_UDT[kw], random_lengths(m, rng, hi=max(2, min(500, m))), rng, sort=False) if kw else None
                run_scan(dev, kbits, vname, values_for(vname, SUM, m, rng), SUM, work=w)
                run_scan(dev, kbits, vname, values_for(vname, MAX, m, rng), MAX, True, work=w)
            w.check_guard()
        finally:
            w.release()
    # one byte short
    m = 5000
    kin = Guarded(dev, rng.integers(0, 99, size=m).astype(np.uint32), seed=1)
    vin = Guarded(dev, rng.integers(0, 99, size=m).astype(np.uint32), seed=2)
    sent = sentinels(np.uint32, m, 7)
    out = Guarded(dev, sent, seed=3)
    wb = scan_bytes(dev, 4, 0, m)
    w = Guarded(dev, nbytes=wb, seed=4)
    try:
        for kw in (0, 4):
            rc = call_scan(dev, kw, kin.ptr(), 0, SUM, 0, None, vin.ptr(), out.ptr(), m, w.ptr(), wb - 1)
            assert rc == 1 and str(wb) in lib_err(), lib_err()
        assert np.array_equal(out.read(np.uint32), sent)
    finally:
        for b in (kin, vin, out, w):
            b.release()


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(dev):
    lib = _lib.load()
    I32 = 1
    n = 5000
    rng = np.random.default_rng(71)
    kbits = rng.integers(0, 99, size=n).astype(np.uint32)
    vbits = rng.integers(0, 99, size=n).astype(np.uint32)
    sent = sentinels(np.uint32, n, 9)
    kin, vin, out = Guarded(dev, kbits, seed=1), Guarded(dev, vbits, seed=2), Guarded(dev, sent, seed=3)
    wb = scan_bytes(dev, 4, I32, n)
    w = Guarded(dev, nbytes=wb, seed=4)
    sz = ctypes.c_size_t()
    keep, iptr = host_init(np.uint32(7))

    def refused(rc, what):
        assert rc == 1, what
        msg = lib_err()
        assert msg, what
        return msg

    def by_key(key_bytes=4, keys=0, value_type=I32, op=SUM, exclusive=0, init=None, vals=0, o=0, m=n, work=0, work_bytes=wb):
        """0 = the proper buffer; anything else replaces it"""
        return lib.adlhip_scan_by_key(dev._h, key_bytes, kin.ptr() if keys == 0 else keys, value_type, op, exclusive, init,
                                      vin.ptr() if vals == 0 else vals, out.ptr() if o == 0 else o, m, w.ptr() if work == 0 else work, work_bytes)

    def plain(value_type=I32, op=SUM, exclusive=0, init=None, vals=0, o=0, m=n, work=0, work_bytes=wb):
        return lib.adlhip_scan_typed(dev._h, value_type, op, exclusive, init, vin.ptr() if vals == 0 else vals, out.ptr() if o == 0 else o, m,
                                     w.ptr() if work == 0 else work, work_bytes)

    null = ctypes.c_void_p(0)
    try:
        for fn, label in ((by_key, "scan by key"), (plain, "scan")):
            refused(fn(vals=null), label + ": NULL values")
            refused(fn(o=null), label + ": NULL d_out")
            refused(fn(work=null), label + ": NULL work")
            refused(fn(vals=vin.ptr(8), m=n - 2), label + ": misaligned values")
            refused(fn(o=out.ptr(4), m=n - 1), label + ": misaligned d_out")
            refused(fn(work=w.ptr(4), work_bytes=wb - 4), label + ": misaligned work")
            refused(fn(o=vin.ptr(16), m=n - 4), label + ": d_out overlaps the values partially")
            refused(fn(vals=out.ptr(32), m=n - 8), label + ": the values overlap d_out partially")
            refused(fn(m=1 << 32), label + ": n = 2^32")
            for bad in (-1, 6, 99):
                refused(fn(value_type=bad), label + ": value_type %d" % bad)
            for bad in (-1, 3):
                refused(fn(op=bad), label + ": op %d" % bad)
            for bad in (-1, 2):
                refused(fn(exclusive=bad), label + ": exclusive %d" % bad)
            refused(fn(init=iptr), label + ": an init with an inclusive scan")
            refused(fn(init=iptr, m=0), label + ": an init with an inclusive scan of nothing")
            assert str(wb) in refused(fn(work_bytes=wb - 1), label + ": work one byte short")
        refused(by_key(keys=null), "NULL keys")
        refused(by_key(keys=kin.ptr(4), m=n - 1), "misaligned keys")
        refused(by_key(o=kin.ptr(0)), "d_out is the keys")
        refused(by_key(o=kin.ptr(16), m=n - 4), "d_out overlaps the keys")
        for bad in (0, 2, 16, -4):
            refused(by_key(key_bytes=bad), "key_bytes %d" % bad)
            refused(lib.adlhip_scan_by_key_scratch_bytes(dev._h, bad, I32, n, ctypes.byref(sz)), "scratch, key_bytes %d" % bad)
        for bad in (-1, 6, 99):
            refused(lib.adlhip_scan_by_key_scratch_bytes(dev._h, 4, bad, n, ctypes.byref(sz)), "scratch, value_type %d" % bad)
            refused(lib.adlhip_scan_typed_scratch_bytes(dev._h, bad, n, ctypes.byref(sz)), "scratch, value_type %d" % bad)
        assert np.array_equal(out.read(np.uint32), sent), "d_out was written"
        assert np.array_equal(kin.read(np.uint32), kbits) and np.array_equal(vin.read(np.uint32), vbits)
        w.check_guard()
        assert dev.getParam("debug.idle_dirty") == 0
        # the proper call goes through, with an init too
        assert by_key(exclusive=1, init=iptr) == 0, lib_err()
        assert np.array_equal(out.read(np.uint32), scan_oracle(kbits, vbits, "i32", SUM, True, np.uint32(7)))
    finally:
        for b in (kin, vin, out, w):
            b.release()


# ---------------------------------------------------------------------------------------------
# call sequences
# ---------------------------------------------------------------------------------------------
def test_call_sequences(dev):
    """scans mixed with a sort, unique, reduceByKey and top-k on one handle; the handle's device state is idle after each step"""
    n = 90_001
    rng = np.random.default_rng(43)
    kbits = np.sort(rng.integers(0, 1 << 12, size=n).astype(np.uint64))
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    p = Pprims()
    sort_buf = Buffer(dev, n, np.uint32)
    fkeys = Buffer(dev, n, np.float32)
    fvals = Buffer(dev, n, np.float32)
    try:
        run_scan(dev, kbits, "f32", values_for("f32", SUM, n, rng), SUM)
        assert dev.getParam("debug.idle_dirty") == 0
        sort_buf.write(keys)
        p.radixSort(dev, sort_buf, n)
        assert np.array_equal(sort_buf.toHost(), np.sort(keys))
        assert dev.getParam("debug.idle_dirty") == 0
        run_scan(dev, None, "i64", values_for("i64", MAX, n, rng), MAX, True)
        assert dev.getParam("debug.idle_dirty") == 0
        fkeys.write(keys.view(np.float32))
        res = p.unique(dev, fkeys, n, counts=True)
        assert int(res.count.toHost()[0]) == np.unique(keys).size
        for b in (res.unique, res.counts, res.count):
            b.release()
        assert dev.getParam("debug.idle_dirty") == 0
        run_scan(dev, kbits.astype(np.uint32), "f64", values_for("f64", SUM, n, rng), SUM, True, init_for("f64", SUM, rng))
        assert dev.getParam("debug.idle_dirty") == 0
        fvals.write(rng.integers(-8, 9, size=n).astype(np.float32))
        res = p.reduceByKey(dev, fkeys, fvals, n, op="sum")
        assert int(res.count.toHost()[0]) == np.unique(keys).size
        for b in (res.unique, res.reduced, res.count):
            b.release()
        assert dev.getParam("debug.idle_dirty") == 0
        run_scan(dev, kbits, "u32", values_for("u32", MIN, n, rng), MIN, in_place=True, exp=None)
        assert dev.getParam("debug.idle_dirty") == 0
        idx = p.topk(dev, sort_buf, n, 100)
        assert np.array_equal(idx.toHost(), np.arange(100, dtype=np.uint32))       # sort_buf is sorted
        idx.release()
        assert dev.getParam("debug.idle_dirty") == 0
        run_scan(dev, None, "f32", values_for("f32", SUM, n, rng), SUM)
        assert dev.getParam("debug.idle_dirty") == 0
    finally:
        for b in (sort_buf, fkeys, fvals):
            b.release()
        p.close()


# ---------------------------------------------------------------------------------------------
# Python mirror, torch front end, the facade's device path
# ---------------------------------------------------------------------------------------------
def test_pprims_mirror(dev):
    n = 60_007
    rng = np.random.default_rng(81)
    kbits = np.repeat(rng.integers(0, 777, size=n).astype(np.uint64) * np.uint64(0x0010000000000001), rng.integers(1, 50, size=n))[:n]
    vals = rng.integers(-8, 9, size=n).astype(np.float32)
    vbits = vals.view(np.uint32)
    p = Pprims()
    keys, src, dst = Buffer(dev, n, np.float64), Buffer(dev, n, np.float32), Buffer(dev, n, np.float32)
    try:
        keys.write(kbits.view(np.float64))
        for op, code in (("sum", SUM), ("min", MIN), ("max", MAX)):
            src.write(vals)
            p.scanByKey(dev, keys, dst, src, n, op=op)
            assert np.array_equal(dst.toHost().view(np.uint32), scan_oracle(kbits, vbits, "f32", code))
            p.scanTyped(dev, dst, src, n, op=op, exclusive=True)
            assert np.array_equal(dst.toHost().view(np.uint32), scan_oracle(None, vbits, "f32", code, True))
            p.scanByKey(dev, keys, dst, src, n, op=op, exclusive=True, init=2.0)
            assert np.array_equal(dst.toHost().view(np.uint32), scan_oracle(kbits, vbits, "f32", code, True, np.float32(2.0).view(np.uint32)))
            assert np.array_equal(src.toHost(), vals) and np.array_equal(keys.toHost().view(np.uint64), kbits)
            p.scanByKey(dev, keys, src, src, n, op=op)                                     # dst is src
            assert np.array_equal(src.toHost().view(np.uint32), scan_oracle(kbits, vbits, "f32", code))
            src.write(vals)
            p.scanTyped(dev, src, src, n, op=op)
            assert np.array_equal(src.toHost().view(np.uint32), scan_oracle(None, vbits, "f32", code))
        # the first m elements only; nothing at all
        src.write(vals)
        dst.write(np.full(n, -1.0, np.float32))
        p.scanTyped(dev, dst, src, 1000)
        got = dst.toHost()
        assert np.array_equal(got[:1000].view(np.uint32), scan_oracle(None, vbits[:1000], "f32", SUM)) and (got[1000:] == -1.0).all()
        p.scanByKey(dev, keys, dst, src, 0)
        assert np.array_equal(dst.toHost(), got)
        with pytest.raises(Exception):
            p.scanTyped(dev, dst, src, n, op="mean")
        with pytest.raises(Exception):
            p.scanTyped(dev, dst, src, n, init=1.0)
    finally:
        for b in (keys, src, dst):
            b.release()
        p.close()
    assert dev.getParam("debug.idle_dirty") == 0


@pytest.fixture(scope="module")
def sorter():
    from oclradixsort_amd import TorchSorter
    s = TorchSorter(0)
    yield s
    s.close()


_DTYPES = ["int32", "int64", "float32", "float64"]


def _torch_values(dtype, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if dtype.is_floating_point:       # multiples of 0.25 whose sums stay exact; no zero (so no -0), no NaN
        t = torch.randint(-40, 40, (n,), dtype=torch.int64, device="cuda", generator=g)
        return torch.where(t == 0, torch.ones_like(t), t).to(dtype) * 0.25
    info = torch.iinfo(dtype)
    return torch.randint(info.min, info.max, (n,), dtype=dtype, device="cuda", generator=g)       # sums wrap


@pytest.mark.parametrize("dtype_name", _DTYPES)
def test_torch_sorter_cumsum_cummax_cummin_match_torch(sorter, dtype_name):
    dt = getattr(torch, dtype_name)
    n = 50_003
    t = _torch_values(dt, n, 11)
    keep = t.clone()
    for x in (t, t[::2], t[1:], t[:1], t[:0]):
        got = sorter.cumsum(x)
        assert got.dtype == dt and got.shape == x.shape
        assert torch.equal(got, torch.cumsum(x, 0, dtype=dt))
        if x.numel():
            assert torch.equal(sorter.cummax(x), torch.cummax(x, 0).values) and torch.equal(sorter.cummin(x), torch.cummin(x, 0).values)
        else:
            assert sorter.cummax(x).numel() == 0 and sorter.cummin(x).dtype == dt
    assert torch.equal(t, keep), "the input was changed"


@pytest.mark.parametrize("vdtype_name", _DTYPES)
@pytest.mark.parametrize("kdtype_name", _DTYPES)
def test_torch_sorter_scan_by_key_matches_per_group_torch(sorter, kdtype_name, vdtype_name):
    kd, vd = getattr(torch, kdtype_name), getattr(torch, vdtype_name)
    n = 20_011
    g = torch.Generator(device="cuda").manual_seed(5)
    lengths = torch.randint(1, 400, (300,), device="cuda", generator=g)
    keys = torch.repeat_interleave(torch.randint(-50, 50, (300,), device="cuda", generator=g), lengths)[:n].to(kd)
    assert keys.numel() == n
    vals = _torch_values(vd, n, 12)
    keep_k, keep_v = keys.clone(), vals.clone()
    for k, v in ((keys, vals), (keys[::2], vals[::2]), (keys[1:], vals[1:])):
        _, counts = torch.unique_consecutive(k, return_counts=True)
        groups = torch.split(v, counts.tolist())
        want = {"sum": torch.cat([torch.cumsum(s, 0, dtype=vd) for s in groups]),
                "max": torch.cat([torch.cummax(s, 0).values for s in groups]),
                "min": torch.cat([torch.cummin(s, 0).values for s in groups])}
        for op in ("sum", "min", "max"):
            got = sorter.scan_by_key(k, v, op=op)
            assert got.dtype == vd and torch.equal(got, want[op]), op
        # exclusive, with an init: the init at every group's first element, init + the inclusive value in front elsewhere
        starts = torch.cumsum(counts, 0) - counts
        got = sorter.scan_by_key(k, v, exclusive=True, init=3)
        exp = torch.roll(want["sum"], 1) + 3
        exp[starts] = 3
        assert torch.equal(got, exp.to(vd))
        got = sorter.scan_by_key(k, v, exclusive=True)
        exp = torch.roll(want["sum"], 1)
        exp[starts] = 0
        assert torch.equal(got, exp)
    assert torch.equal(keys, keep_k) and torch.equal(vals, keep_v), "an input was changed"
    e = sorter.scan_by_key(torch.empty(0, dtype=kd, device="cuda"), torch.empty(0, dtype=vd, device="cuda"))
    assert e.numel() == 0 and e.dtype == vd


def test_torch_sorter_scans_are_bound_to_their_stream(sorter, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a native call was made")

    k = torch.tensor([3, 3, 1, 1, 1, 3], dtype=torch.int32, device="cuda")
    v = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 32.0], dtype=torch.float64, device="cuda")
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        monkeypatch.setattr(sorter.pprims, "scanTyped", boom)
        monkeypatch.setattr(sorter.pprims, "scanByKey", boom)
        for call in (lambda: sorter.cumsum(v), lambda: sorter.cummax(v), lambda: sorter.cummin(v), lambda: sorter.scan_by_key(k, v)):
            with pytest.raises(RuntimeError):
                call()
        monkeypatch.undo()
    assert sorter.cumsum(v).tolist() == [1.0, 3.0, 7.0, 15.0, 31.0, 63.0]
    assert sorter.scan_by_key(k, v).tolist() == [1.0, 3.0, 4.0, 12.0, 28.0, 32.0]
    assert sorter.scan_by_key(k, v, op="max", exclusive=True, init=5.0).tolist() == [5.0, 5.0, 5.0, 5.0, 8.0, 5.0]
    assert sorter.cummin(-v).tolist() == (-v).tolist() and sorter.cummax(-v).tolist() == [-1.0] * 6
    i32 = torch.tensor([2 ** 31 - 1, 1, 5], dtype=torch.int32, device="cuda")
    assert sorter.cumsum(i32).tolist() == [2 ** 31 - 1, -2 ** 31, -2 ** 31 + 5]       # wraps in the input's dtype
    for bad in (torch.zeros(6, dtype=torch.float16, device="cuda"), torch.zeros(6, dtype=torch.float32), [3.0, 1.0],
                torch.zeros((2, 3), dtype=torch.int32, device="cuda")):
        for call in (sorter.cumsum, sorter.cummax, sorter.cummin, lambda b: sorter.scan_by_key(b, v), lambda b: sorter.scan_by_key(k, b)):
            with pytest.raises((TypeError, ValueError)):
                call(bad)
    with pytest.raises(ValueError):
        sorter.scan_by_key(k, torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        sorter.scan_by_key(k, v, op="mean")
    with pytest.raises(ValueError):
        sorter.scan_by_key(k, v, init=1.0)          # inclusive


def test_scan_demo_device_path_matches_its_host_path():
    demo = os.path.join(ROOT, "tests", "demo", "scan_demo")

    def lines(args):
        r = subprocess.run([demo] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return [ln for ln in r.stdout.splitlines() if ln.strip()]

    device, host = lines(["--dump"]), lines(["--host", "--dump"])
    assert len(device) == len(host) and len([ln for ln in device if ln.startswith("DUMP ")]) == 9 * 3 * 2 * 3
    assert all(ln.startswith("[ OK ] Scan.") for ln in device if ln.startswith("["))
    assert device == host
