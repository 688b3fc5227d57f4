"""Every primitive past 2^31 elements and 2^32 bytes on the device (include/adlhip.h; DESIGN.md "Index widths at the top of the range").

The inputs are the closed forms of tests/large_n.py (checked against numpy on the CPU by tests/test_large_n_forms.py); they are
generated on the device, the results are verified on the device chunk by chunk, and nothing but a few words per chunk is read back.
Everything goes through the C ABI with ctypes, on a handle bound to torch's current stream.  All device memory of a case is carved
out of ONE arena -- one torch allocation for the module, regions 256-byte aligned --; every output and the work buffer have 4 KiB
of canary on both sides, the work buffer is exactly the bytes the *_scratch_bytes function reports and is prefilled with junk, and
the inputs are compared with their regenerated forms after the call.  After each case adlhip_fault_check is clean and
"debug.idle_dirty" is 0.

Sizes: N31 = 2^31 + 12345 (an index past the sign bit), N30 = 2^30 + 12345 (byte offsets of 4-byte elements past 2^32; used where the
case at N31 would need more than the arena, which is said in the test's name), NB8 = 2^29 + 4321 (8-byte elements), NB16 = 2^28 +
4321 (16-byte values), NMAX = 0xFFF00000 (the limit).  The arena is ARENA_BYTES = 80 GiB; with the temporaries of generation and
verification (chunks of 2^26 int64) a case stays below 96 GiB, which every case asserts.  The fixture FAILS when the device has less
free memory than that; it never skips.

At N30 instead of N31, because the case at N31 needs more than the arena: the flat paths of sort_rows and sort_segments and unique with
indices -- their work is the argsort's (32 n bytes) and four or five arrays of n elements besides.  Not here: the per-row loop of
topk_rows, a dozen launches per row, with 2^18 rows and more.

Measured on an MI355X (generation, call and verification; peak = arena in use + what torch reserved for the verifier's temporaries):
  case                                                      peak GiB   seconds
  radix_sort u32 N31 / NMAX                                 24.9 / 40.9   0.5 / 0.2
  radix_sort kv32, soa32 N31                                43.7          0.3
  radix_sort u64 NB8; soa 8/16 NB16                         19.7; 27.7    0.1; 0.3
  sort_keys_typed i32 N31                                   28.4          0.2
  argsort_typed i32 / f32 N31 (the largest cases)           67.8 / 69.3   0.4 / 0.6
  argsort_typed i64 / f64 NB8; sort_pairs f64/16 NB16       31.3; 29.2    0.1 - 0.2
  key codec f32 NMAX / f64 NB8                              39.5 / 15.5   0.7 / 0.1
  topk f32 N31 (4 cases), all-equal N31; f64 NB8            69.3; 31.3    0.1 - 0.3
  sort_rows 32 columns (2); topk_rows 32 columns            31.5; 18.0    0.3; 0.6
  sort_rows 4099 columns; topk_rows 4099 columns            61.3; 15.6    0.3; 0.2
  sort_segments plan / flat                                 32.1 / 57.8   1.1 / 0.6
  unique i32 N30 / i64 NB8; run_length_encode NMAX          61.8 / 43.8; 72.0   0.1 - 0.2
  reduce_runs N31 (3); reduce_by_key NB8                    72.0; 49.8    0.2; 0.1
  scans (6 cases)                                           16.0 - 40.0   0.0 - 0.3
  compact flagged / if (2) NMAX                             60.0 / 56.0   0.3 - 0.4
  bincount (3), histogram_range (3)                         12.0 - 62.4   0.0 - 0.3
  merge NMAX / past 2^31 with values                        56.0 / 48.0   0.9 / 0.6
  set operations (4); search (4)                            25.2 - 32.6; 16.0 - 24.0   0.1 - 0.3
  scratch sizes (27 cases, host only)                       0             0.0
The whole module: 21 s, its slowest case 1.1 s.  The yardstick, test_gpu_parity.py::test_u32_2p30_plus_12345_three_kernel_path_and_large_sort,
takes 10.7 s on the same machine.
"""
import ctypes
import time

import pytest
import torch  # before the HIP back-end is loaded

import large_n as L
from oclradixsort_amd import DeviceUtils, _lib

pytestmark = pytest.mark.gpu

GiB = 1 << 30
ARENA_BYTES = 80 * GiB
LIMIT_BYTES = 96 * GiB
GUARD = 4096
CANARY, JUNK, SENTINEL = 0xC5, 0xA7, 0x5A
N31, N30, NB8, NB16, NMAX = (1 << 31) + 12345, (1 << 30) + 12345, (1 << 29) + 4321, (1 << 28) + 4321, 0xFFF00000
U32, I32, F32, U64, I64, F64 = range(6)
ASC, DESC = L.ASC, L.DESC
SUM, MIN, MAX = 0, 1, 2
I4, I8 = torch.int32, torch.int64


class Arena:
    """regions of one allocation; guarded regions have GUARD bytes of canary directly in front and directly behind"""

    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        self.reset()

    def reset(self):
        self.off, self.guards = 0, []

    def _fit(self, end):
        if end > self.buf.numel():
            pytest.fail("the case needs more than the arena: %d bytes of %d" % (end, self.buf.numel()))

    def take(self, n, dtype, name, guarded=True, prefill=None):
        """n elements of dtype at a 256-byte boundary; an output (guarded) has its canaries directly in front and directly behind and is
        prefilled with SENTINEL bytes"""
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        front = GUARD if guarded else 0
        start = (self.off + front + 255) // 256 * 256
        end = start + nbytes + front
        self._fit(end)
        self.off = end
        if guarded:
            for g, side in ((start - GUARD, " (front)"), (start + nbytes, " (back)")):
                self.buf[g:g + GUARD] = CANARY
                self.guards.append((name + side, g))
        raw = self.buf[start:start + nbytes]
        if prefill is not None or guarded:
            raw.fill_(SENTINEL if prefill is None else prefill)
        return raw.view(dtype)

    def check_guards(self):
        for name, off in self.guards:
            bad = self.buf[off:off + GUARD] != CANARY
            if bool(bad.any()):
                raise AssertionError("canary of %s overwritten at byte %d of it" % (name, int(bad.nonzero()[0, 0])))


class Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.dev = DeviceUtils.allocate(stream=torch.cuda.current_stream().cuda_stream)
        self.h = self.dev._h
        free, total = torch.cuda.mem_get_info()
        if free < LIMIT_BYTES:
            pytest.fail("the large-n cases need %d bytes of device memory (an arena of %d and the verifier's temporaries); %d of %d are "
                        "free" % (LIMIT_BYTES, ARENA_BYTES, free, total))
        self.arena = Arena(ARENA_BYTES)
        self.keep = []

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.h, *args)
        if rc != 0:
            raise AssertionError("%s failed: %s" % (name, (self.lib.adlhip_last_error() or b"?").decode()))

    def refused(self, name, *args):
        return getattr(self.lib, name)(self.h, *args) != 0

    def size(self, name, *args, outs=1):
        """a *_scratch_bytes call; returns its size_t outputs"""
        vals = [ctypes.c_size_t(0) for _ in range(outs)]
        self.call(name, *args, *[ctypes.byref(v) for v in vals])
        return [v.value for v in vals] if outs > 1 else vals[0].value

    def work(self, nbytes):
        """the work buffer: exactly nbytes, guarded, junk inside"""
        return self.arena.take(max(nbytes, 0), torch.uint8, "work", prefill=JUNK), nbytes

    def host(self, value, ctype):
        v = ctype(value)
        self.keep.append(v)
        return ctypes.cast(ctypes.pointer(v), ctypes.c_void_p)

    def begin(self):
        self.arena.reset()
        self.keep = []
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()

    def end(self, what):
        """after the last check of a case: the canaries, the fault word, the idle state, the memory condition"""
        assert self.lib.adlhip_fault_check(self.h) == 0, self.lib.adlhip_last_error()
        torch.cuda.synchronize()
        assert self.lib.adlhip_fault_check(self.h) == 0, self.lib.adlhip_last_error()
        self.arena.check_guards()
        assert self.dev.getParam("debug.idle_dirty") == 0
        peak = self.arena.off + torch.cuda.max_memory_reserved() - ARENA_BYTES
        print("%s: arena %.1f GiB, peak device bytes %.1f GiB, %.1f s" % (what, self.arena.off / GiB, peak / GiB, time.perf_counter() - self.t0))
        assert peak <= LIMIT_BYTES, (what, peak)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def cx():
    old = L.CHUNK
    L.CHUNK = 1 << 26
    c = Ctx()
    yield c
    c.arena = None
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    DeviceUtils.deallocate(c.dev)
    L.CHUNK = old


@pytest.fixture(autouse=True)
def _case(cx):
    cx.begin()
    yield


def identity(j):
    return j


def high_half(t):
    return (t >> 32) & L.M32


# ---------------------------------------------------------------------------------------------------------------------
# plain sorts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N31, NMAX], ids=["N31", "NMAX"])
def test_radix_sort_u32(cx, n):
    """whole u32 keys, a permutation of 0 .. n - 1: the sorted keys are the positions"""
    p = L.Perm(n)
    tmp_b, work_b = cx.size("adlhip_radix_sort_scratch_bytes", 0, n, outs=2)
    keys = L.fill(cx.arena.take(n, I4, "keys"), p)
    tmp = cx.arena.take(tmp_b // 4, I4, "tmp")
    work, wb = cx.work(work_b)
    cx.call("adlhip_radix_sort_u32", P(keys), P(tmp), P(work), wb, n, 32)
    L.check_equal(keys, identity, n, "sorted keys")
    cx.end("radix_sort_u32 n=%d" % n)


def test_radix_sort_kv32_N31(cx):
    """pairs {key = P(i) >> 3, value = i}: ties, so the values are pinned by the gather and rising properties"""
    n = N31
    f = L.SortForm(n, "u32", ASC, 3, base=0)
    tmp_b, work_b = cx.size("adlhip_radix_sort_scratch_bytes", 1, n, outs=2)
    pairs = L.fill(cx.arena.take(n, I8, "pairs"), lambda i: f.keys_in(i) | (i << 32))
    tmp = cx.arena.take(tmp_b // 8, I8, "tmp")
    work, wb = cx.work(work_b)
    cx.call("adlhip_radix_sort_kv32", P(pairs), P(tmp), P(work), wb, n, 32)
    L.check_gather(pairs, f.keys_in, f.keys_out, n, n, "values", conv=high_half)
    L.check_rising(pairs, f.keys_out, n, "values", conv=high_half)
    for lo, hi in L.chunks(n):   # the key halves
        k = pairs[lo:hi] & L.M32
        assert bool((k == f.keys_out(L.arange(lo, hi, k.device))).all()), "keys of the pairs in [%d, %d)" % (lo, hi)
    cx.end("radix_sort_kv32 n=%d" % n)


def test_radix_sort_u64_NB8(cx):
    """8-byte keys whose dwords both vary, byte offsets past 2^32"""
    n = NB8
    f = L.SortForm(n, "u64")
    tmp_b, work_b = cx.size("adlhip_radix_sort_scratch_bytes", 2, n, outs=2)
    keys = L.fill(cx.arena.take(n, I8, "keys"), f.keys_in)
    tmp = cx.arena.take(tmp_b // 8, I8, "tmp")
    work, wb = cx.work(work_b)
    cx.call("adlhip_radix_sort_u64", P(keys), P(tmp), P(work), wb, n, 64)
    L.check_equal(keys, f.keys_out, n, "sorted keys")
    cx.end("radix_sort_u64 n=%d" % n)


def test_radix_sort_soa32_N31(cx):
    """separate key and value arrays, ties"""
    n = N31
    f = L.SortForm(n, "u32", ASC, 3, base=0)
    tmp_b, work_b = cx.size("adlhip_radix_sort_scratch_bytes", 3, n, outs=2)
    keys = L.fill(cx.arena.take(n, I4, "keys"), f.keys_in)
    vals = L.fill(cx.arena.take(n, I4, "vals"), identity)
    tk, tv = cx.arena.take(tmp_b // 4, I4, "tmp keys"), cx.arena.take(tmp_b // 4, I4, "tmp vals")
    work, wb = cx.work(work_b)
    cx.call("adlhip_radix_sort_soa32", P(keys), P(vals), P(tk), P(tv), P(work), wb, n, 32)
    L.check_equal(keys, f.keys_out, n, "sorted keys")
    L.check_gather(vals, f.keys_in, f.keys_out, n, n, "values")
    L.check_rising(vals, f.keys_out, n, "values")
    cx.end("radix_sort_soa32 n=%d" % n)


def wide_value(e):
    """element e of an array of 16-byte values as two int64: {position, its complement}"""
    i = e >> 1
    return torch.where((e & 1) == 0, i, ~i)


def test_radix_sort_soa_wide_NB16(cx):
    """8-byte keys and 16-byte values: the values' byte offsets pass 2^32; distinct keys, so the values have a closed form"""
    n = NB16
    f = L.SortForm(n, "u64")
    tk_b, tv_b, work_b = cx.size("adlhip_radix_sort_soa_scratch_bytes", 8, 16, n, 64, outs=3)
    keys = L.fill(cx.arena.take(n, I8, "keys"), f.keys_in)
    vals = L.fill(cx.arena.take(2 * n, I8, "vals"), wide_value)
    tk, tv = cx.arena.take(tk_b // 8, I8, "tmp keys"), cx.arena.take(tv_b // 8, I8, "tmp vals")
    work, wb = cx.work(work_b)
    cx.call("adlhip_radix_sort_soa", P(keys), 8, P(vals), 16, P(tk), P(tv), P(work), wb, n, 64)
    L.check_equal(keys, f.keys_out, n, "sorted keys")
    L.check_equal(vals, lambda e: torch.where((e & 1) == 0, f.index_out(e >> 1), ~f.index_out(e >> 1)), 2 * n, "values")
    cx.end("radix_sort_soa 8/16 n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# typed sorts, argsort, pairs
# ---------------------------------------------------------------------------------------------------------------------
def test_sort_keys_typed_i32_descending_N31(cx):
    """encode, unsigned sort, decode, in place, an index past the sign bit; keys of both signs"""
    n = N31
    f = L.SortForm(n, "i32", DESC)
    tk_b, tv_b, work_b = cx.size("adlhip_sort_typed_scratch_bytes", I32, 0, 0, n, outs=3)
    keys = L.fill(cx.arena.take(n, I4, "keys"), f.keys_in)
    tmp = cx.arena.take(tk_b // 4, I4, "tmp")
    work, wb = cx.work(work_b)
    cx.call("adlhip_sort_keys_typed", I32, DESC, P(keys), P(tmp), P(work), wb, n)
    L.check_equal(keys, f.keys_out, n, "sorted keys")
    cx.end("sort_keys_typed i32 desc n=%d" % n)


@pytest.mark.parametrize("ktype,order,shift,n", [("i32", ASC, 0, N31), ("f32", DESC, 3, N31), ("i64", ASC, 0, NB8), ("f64", DESC, 3, NB8)],
                         ids=["i32-asc-distinct-N31", "f32-desc-ties-N31", "i64-asc-distinct-NB8", "f64-desc-ties-NB8"])
def test_argsort_typed(cx, ktype, order, shift, n):
    """distinct keys: the index is P's inverse; ties: the gather and rising properties pin the stable order.  At N31 the largest case of
    the module: 67 GiB of arena."""
    f = L.SortForm(n, ktype, order, shift)
    dt = I4 if L.key_bytes(ktype) == 4 else I8
    code = L.KEY_TYPES[ktype]
    _, _, work_b = cx.size("adlhip_sort_typed_scratch_bytes", code, 2, 0, n, outs=3)
    kin = L.fill(cx.arena.take(n, dt, "keys in", guarded=False), f.keys_in)
    kout, index = cx.arena.take(n, dt, "keys out"), cx.arena.take(n, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_argsort_typed", code, order, P(kin), P(kout), P(index), P(work), wb, n)
    L.check_equal(kout, f.keys_out, n, "sorted keys")
    if shift == 0:
        L.check_equal(index, f.index_out, n, "index")
    else:
        L.check_gather(index, f.keys_in, f.keys_out, n, n, "index")
        L.check_rising(index, f.keys_out, n, "index")
    L.check_equal(kin, f.keys_in, n, "the input afterwards")
    cx.end("argsort_typed %s n=%d" % (ktype, n))


def test_sort_pairs_typed_f64_wide_values_NB16(cx):
    """8-byte float keys of both signs, 16-byte values, descending, in place"""
    n = NB16
    f = L.SortForm(n, "f64", DESC)
    tk_b, tv_b, work_b = cx.size("adlhip_sort_typed_scratch_bytes", F64, 1, 16, n, outs=3)
    keys = L.fill(cx.arena.take(n, I8, "keys"), f.keys_in)
    vals = L.fill(cx.arena.take(2 * n, I8, "vals"), wide_value)
    tk, tv = cx.arena.take(tk_b // 8, I8, "tmp keys"), cx.arena.take(tv_b // 8, I8, "tmp vals")
    work, wb = cx.work(work_b)
    cx.call("adlhip_sort_pairs_typed", F64, DESC, P(keys), P(vals), 16, P(tk), P(tv), P(work), wb, n)
    L.check_equal(keys, f.keys_out, n, "sorted keys")
    L.check_equal(vals, lambda e: torch.where((e & 1) == 0, f.index_out(e >> 1), ~f.index_out(e >> 1)), 2 * n, "values")
    cx.end("sort_pairs_typed f64/16 n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# key codec
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ktype,n", [("f32", NMAX), ("f64", NB8)], ids=["f32-NMAX", "f64-NB8"])
def test_key_codec(cx, ktype, n):
    """the code of a key is its ordinal as an unsigned number (descending: the complement), stated without the codec's formula; decode
    gives the keys back, in place"""
    f = L.SortForm(n, ktype)
    code = L.KEY_TYPES[ktype]
    if ktype == "f32":
        dt, want = I4, (lambda i: ~(f.base + f.rank_in(i)))
    else:
        dt, want = I8, (lambda i: ~((f.rank_in(i) * f.C8 + f.D8) ^ L.MIN64))
    src = L.fill(cx.arena.take(n, dt, "src", guarded=False), f.keys_in)
    dst = cx.arena.take(n, dt, "dst")
    cx.call("adlhip_key_encode", code, DESC, P(dst), P(src), n)
    L.check_equal(dst, want, n, "codes")
    L.check_equal(src, f.keys_in, n, "the input afterwards")
    cx.call("adlhip_key_decode", code, DESC, P(dst), P(dst), n)
    L.check_equal(dst, f.keys_in, n, "decoded keys")
    cx.end("key codec %s n=%d" % (ktype, n))


# ---------------------------------------------------------------------------------------------------------------------
# top-k
# ---------------------------------------------------------------------------------------------------------------------
K_SMALL, K_LARGE = 1000, (1 << 20) + 3


def run_topk(cx, ktype, order, n, k, algo, in_form, out_form, index_form, what):
    code = L.KEY_TYPES[ktype]
    dt = I4 if L.key_bytes(ktype) == 4 else I8
    work_b = cx.size("adlhip_topk_scratch_bytes", code, n, k)
    kin = L.fill(cx.arena.take(n, dt, "keys in", guarded=False), in_form)
    kout, index = cx.arena.take(k, dt, "keys out"), cx.arena.take(k, I4, "index")
    work, wb = cx.work(work_b)
    cx.dev.setParam("topk.algo", algo)
    try:
        cx.call("adlhip_topk_typed", code, order, P(kin), n, k, P(kout), P(index), P(work), wb)
    finally:
        cx.dev.setParam("topk.algo", -1)
    L.check_equal(kout, out_form, k, what + " keys")
    L.check_equal(index, index_form, k, what + " index")
    L.check_equal(kin, in_form, n, "the input afterwards")
    cx.end("topk %s n=%d k=%d algo=%d" % (what, n, k, algo))


@pytest.mark.parametrize("algo", [1, 0], ids=["select", "sort"])
@pytest.mark.parametrize("k", [K_SMALL, K_LARGE])
def test_topk_f32_N31(cx, k, algo):
    """the k largest of distinct float keys of both signs; selection (32 position bits) and full argsort"""
    f = L.SortForm(N31, "f32", DESC)
    run_topk(cx, "f32", DESC, N31, k, algo, f.keys_in, f.keys_out, f.index_out, "f32 desc")


def test_topk_all_equal_keys_N31(cx):
    """all keys equal: the key digits decide nothing and the selection descends through all three position digits of select_plan's
    pos_bits = 32 (n > 2^31: 11 + 11 + 10 bits); the result is the first k positions"""
    run_topk(cx, "i32", ASC, N31, K_LARGE, 1, lambda i: torch.full_like(i, 0xfffffff9), lambda j: torch.full_like(j, 0xfffffff9), identity,
             "all equal")


def test_topk_f64_NB8(cx):
    f = L.SortForm(NB8, "f64", ASC)
    run_topk(cx, "f64", ASC, NB8, K_SMALL, 1, f.keys_in, f.keys_out, f.index_out, "f64 asc")


# ---------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------
ROWS32 = (1 << 26) + 386        # x 32 columns = 2^31 + 12352 elements


@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
def test_sort_rows_32_columns_past_2p31(cx, order):
    """the row kernel, 128 rows per tile; the last tile is partial"""
    r = L.Rows32(ROWS32, order)
    n = ROWS32 * 32
    work_b = cx.size("adlhip_sort_rows_scratch_bytes", I32, ROWS32, 32)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), r.keys_in)
    kout, index = cx.arena.take(n, I4, "keys out"), cx.arena.take(n, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_sort_rows_typed", I32, order, P(kin), ROWS32, 32, 32, P(kout), P(index), P(work), wb)
    L.check_equal(kout, r.keys_out, n, "sorted rows")
    L.check_equal(index, r.index_out, n, "columns")
    L.check_equal(kin, r.keys_in, n, "the input afterwards")
    cx.end("sort_rows 32 columns n=%d" % n)


def test_topk_rows_32_columns_past_2p31(cx):
    """k = 5 of 32 columns: the outputs' row r starts at 5 r, the input's at 32 r past 2^31"""
    r, k = L.Rows32(ROWS32, ASC), 5
    n = ROWS32 * 32
    work_b = cx.size("adlhip_topk_rows_scratch_bytes", I32, ROWS32, 32, k)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), r.keys_in)
    kout, index = cx.arena.take(ROWS32 * k, I4, "keys out"), cx.arena.take(ROWS32 * k, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_topk_rows_typed", I32, ASC, P(kin), ROWS32, 32, 32, k, P(kout), P(index), P(work), wb)
    flat = lambda e: (e // k) * 32 + e % k   # noqa: E731  (output element e is sorted column e % k of row e // k)
    L.check_equal(kout, lambda e: r.keys_out(flat(e)), ROWS32 * k, "top keys")
    L.check_equal(index, lambda e: r.index_out(flat(e)), ROWS32 * k, "top columns")
    L.check_equal(kin, r.keys_in, n, "the input afterwards")
    cx.end("topk_rows 32 columns n=%d" % n)


PRIME_COLS = 4099
ROWS_PRIME = (1 << 30) // PRIME_COLS + 7   # x 4099 = 2^30 + ~30000 elements


def test_sort_rows_prime_columns_flat_path_strided_N30(cx):
    """4099 columns take the flat path (pack, argsort of all keys, row sort, emit); the input is strided, with poison between the rows.
    About 2^30 elements: the flat path's work is the argsort's."""
    rows, cols, stride = ROWS_PRIME, PRIME_COLS, PRIME_COLS + 5
    r = L.RowsPrime(rows, cols, order=DESC, stride=stride)
    n = rows * cols
    work_b = cx.size("adlhip_sort_rows_scratch_bytes", U32, rows, cols)
    assert work_b > 4 * n
    kin = L.fill(cx.arena.take(rows * stride, I4, "keys in", guarded=False), r.keys_in_strided)
    kout, index = cx.arena.take(n, I4, "keys out"), cx.arena.take(n, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_sort_rows_typed", U32, DESC, P(kin), rows, cols, stride, P(kout), P(index), P(work), wb)
    L.check_equal(kout, r.keys_out, n, "sorted rows")
    check_columns(r, index, n, cols)
    L.check_equal(kin, r.keys_in_strided, rows * stride, "the input afterwards")
    cx.end("sort_rows %d columns n=%d" % (cols, n))


def check_columns(r, index, n_out, cols, out_cols=None):
    """every index is a column of its row that holds the key the form expects there (the keys of a row are distinct)"""
    oc = out_cols or r.cols
    for lo, hi in L.chunks(n_out):
        e = L.arange(lo, hi, index.device)
        f = (e // oc) * r.cols + e % oc
        ix = L.from_u32(index[lo:hi])
        assert bool((ix < cols).all()), "a column out of range in [%d, %d)" % (lo, hi)
        bad = r.key_at_index(f, ix) != r.keys_out(f)
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise L.Mismatch("columns", lo + k, int(ix[k]), "the column of key %d" % int(r.keys_out(f)[k]))


def test_topk_rows_prime_columns_strided_past_2p31(cx):
    """rows longer than the LDS tile: the row kernel's in-kernel selection; rows * stride passes 2^31"""
    cols, stride, k = PRIME_COLS, PRIME_COLS + 5, 7
    rows = (1 << 31) // stride + 11
    r = L.RowsPrime(rows, cols, order=ASC, stride=stride)
    assert rows * stride > (1 << 31)
    work_b = cx.size("adlhip_topk_rows_scratch_bytes", U32, rows, cols, k)
    kin = L.fill(cx.arena.take(rows * stride, I4, "keys in", guarded=False), r.keys_in_strided)
    kout, index = cx.arena.take(rows * k, I4, "keys out"), cx.arena.take(rows * k, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_topk_rows_typed", U32, ASC, P(kin), rows, cols, stride, k, P(kout), P(index), P(work), wb)
    L.check_equal(kout, lambda e: r.keys_out((e // k) * cols + e % k), rows * k, "top keys")
    check_columns(r, index, rows * k, cols, out_cols=k)
    L.check_equal(kin, r.keys_in_strided, rows * stride, "the input afterwards")
    cx.end("topk_rows %d columns, %d rows" % (cols, rows))


# ---------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------
def run_segments(cx, s, index_base, what):
    n, S = s.n, s.S
    work_b = cx.size("adlhip_sort_segments_scratch_bytes", I32, n, S, s.max_segment)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), s.keys_in)
    off = L.fill(cx.arena.take(S + 1, I4, "offsets", guarded=False), s.offsets)
    kout, index = cx.arena.take(n, I4, "keys out"), cx.arena.take(n, I4, "index")
    over = cx.arena.take(4, I4, "oversized")
    work, wb = cx.work(work_b)
    cx.call("adlhip_sort_segments_typed", I32, s.order, P(kin), n, P(off), S, s.max_segment, index_base, P(kout), P(index), P(over), P(work), wb)
    L.check_equal(kout, s.keys_out, n, "sorted segments")
    L.check_count(over, 0, "oversized segments")
    for lo, hi in L.chunks(n):   # the index, by the gather property and, among ties, the rising property
        e = L.arange(lo, hi, index.device)
        start, ln = s.locate(e)
        ix = L.from_u32(index[lo:hi]) - (start if index_base else 0)
        assert bool(((ix >= 0) & (ix < ln)).all()), "an index outside its segment in [%d, %d)" % (lo, hi)
        bad = s.keys_in(start + ix) != s.keys_out(e)
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise L.Mismatch(what + " index", lo + k, int(ix[k]), "a position of key %d" % int(s.keys_out(e)[k]))
        if s.dup and hi - lo > 1:
            w = s.keys_out(e)
            tie = (w[1:] == w[:-1]) & (start[1:] == start[:-1]) & (ix[1:] <= ix[:-1])
            assert not bool(tie.any()), "ties out of order in [%d, %d)" % (lo, hi)
    L.check_equal(kin, s.keys_in, n, "the input afterwards")
    L.check_equal(off, s.offsets, S + 1, "the offsets afterwards")
    cx.end("sort_segments %s n=%d S=%d" % (what, n, S))


def test_sort_segments_plan_path_past_2p31(cx):
    """3.9 Mi segments of every class of the plan, empty ones among them, lengths summing to more than 2^31; ties; global indices"""
    s = L.Segments((1 << 31) // 4441 + 3, order=DESC, dup=1)
    assert s.n > (1 << 31) and s.max_segment == 4096
    run_segments(cx, s, 1, "plan path")


def test_sort_segments_flat_path_N30(cx):
    """one segment of 5003 keys in front sends everything to the flat path; local indices.  About 2^30 elements: the flat path's work is
    the argsort's."""
    s = L.Segments((1 << 30) // 4441 + 3, long_first=5003, order=ASC)
    assert s.n > (1 << 30) and s.max_segment == 5003
    run_segments(cx, s, 0, "flat path")


# ---------------------------------------------------------------------------------------------------------------------
# unique, run-length encode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ktype,n", [("i32", N30), ("i64", NB8)], ids=["i32-N30", "i64-NB8"])
def test_unique_typed_with_counts_inverse_first_index(cx, ktype, n):
    """m = n / 5 + 1 distinct keys, each at positions x, x + m, ...: closed forms for unique, counts, first index and inverse"""
    m = n // 5 + 1
    g = L.Groups(n, m)
    dt = I4 if ktype == "i32" else I8
    code = L.KEY_TYPES[ktype]
    work_b = cx.size("adlhip_unique_scratch_bytes", code, n, 1)
    kin = L.fill(cx.arena.take(n, dt, "keys in", guarded=False), g.key)
    uniq, counts = cx.arena.take(n, dt, "unique"), cx.arena.take(n, I4, "counts")
    first, inverse, num = cx.arena.take(n, I4, "first index"), cx.arena.take(n, I4, "inverse"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_unique_typed", code, ASC, P(kin), n, P(uniq), P(counts), None, P(first), P(inverse), P(num), P(work), wb)
    L.check_count(num, m, "number of unique keys")
    L.check_equal(uniq, identity, m, "unique keys")
    L.check_equal(counts, g.counts, m, "counts")
    L.check_equal(first, g.first_index, m, "first index")
    L.check_equal(inverse, g.key, n, "inverse")
    for t in (uniq, counts, first):   # behind the runs nothing is written
        tail = t[m:n].view(torch.uint8)
        assert bool((tail[:1 << 20] == SENTINEL).all()) and bool((tail[-(1 << 20):] == SENTINEL).all())
    L.check_equal(kin, g.key, n, "the input afterwards")
    cx.end("unique %s n=%d" % (ktype, n))


def test_run_length_encode_NMAX(cx):
    """runs of 5, 5 and 6 keys up to the limit: unique keys and counts"""
    n = NMAX
    r = L.Runs(n)
    work_b = cx.size("adlhip_run_length_encode_scratch_bytes", 4, n)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), r.key)
    uniq, counts, num = cx.arena.take(n, I4, "unique"), cx.arena.take(n, I4, "counts"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_run_length_encode", 4, P(kin), n, P(uniq), P(counts), None, P(num), P(work), wb)
    L.check_count(num, r.num_runs, "number of runs")
    L.check_equal(uniq, identity, r.num_runs, "unique keys")
    L.check_equal(counts, r.counts, r.num_runs, "counts")
    L.check_equal(kin, r.key, n, "the input afterwards")
    cx.end("run_length_encode n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# reduce, scan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [SUM, MIN, MAX], ids=["sum", "min", "max"])
def test_reduce_runs_i64_values_N31(cx, op):
    """4-byte keys in runs, 8-byte values = positions: per-run sum, min and max, offsets"""
    n = N31
    r = L.Runs(n)
    want = {SUM: r.sum_of_positions, MIN: r.min_of_positions, MAX: r.max_of_positions}[op]
    work_b = cx.size("adlhip_reduce_runs_scratch_bytes", 4, I64, n)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), r.key)
    vin = L.fill(cx.arena.take(n, I8, "values in", guarded=False), identity)
    uniq, red = cx.arena.take(n, I4, "unique"), cx.arena.take(n, I8, "reduced")
    offs, num = cx.arena.take(n + 1, I4, "offsets"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_reduce_runs", 4, P(kin), I64, op, P(vin), n, P(uniq), P(red), None, P(offs), P(num), P(work), wb)
    L.check_count(num, r.num_runs, "number of runs")
    L.check_equal(uniq, identity, r.num_runs, "unique keys")
    L.check_equal(red, want, r.num_runs, "reduced values")
    L.check_equal(offs, r.offsets, r.num_runs + 1, "offsets")
    L.check_equal(kin, r.key, n, "the keys afterwards")
    L.check_equal(vin, identity, n, "the values afterwards")
    cx.end("reduce_runs op=%d n=%d" % (op, n))


def test_reduce_by_key_f64_values_NB8(cx):
    """unsorted 8-byte keys, whole-number f64 values = positions: the sum per key is exact (below 2^53) whatever the association"""
    n = NB8
    m = n // 5 + 1
    g = L.Groups(n, m)
    work_b = cx.size("adlhip_reduce_by_key_scratch_bytes", I64, F64, n)
    kin = L.fill(cx.arena.take(n, I8, "keys in", guarded=False), g.key)
    vin = cx.arena.take(n, torch.float64, "values in", guarded=False)
    for lo, hi in L.chunks(n):
        vin[lo:hi] = L.arange(lo, hi, vin.device).to(torch.float64)
    uniq, red = cx.arena.take(n, I8, "unique"), cx.arena.take(n, torch.float64, "reduced")
    counts, num = cx.arena.take(n, I4, "counts"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_reduce_by_key_typed", I64, ASC, P(kin), F64, SUM, P(vin), n, P(uniq), P(red), P(counts), None, P(num), P(work), wb)
    L.check_count(num, m, "number of keys")
    L.check_equal(uniq, identity, m, "unique keys")
    L.check_equal(counts, g.counts, m, "counts")
    for lo, hi in L.chunks(m):
        want = g.sum_of_positions(L.arange(lo, hi, red.device))
        assert int(want.max()) < (1 << 53)
        bad = red[lo:hi] != want.to(torch.float64)
        if bool(bad.any()):
            k = int(bad.nonzero()[0, 0])
            raise L.Mismatch("sums", lo + k, float(red[lo + k]), int(want[k]))
    L.check_equal(kin, g.key, n, "the keys afterwards")
    cx.end("reduce_by_key n=%d" % n)


def test_scan_typed_u32_sum_in_place_NMAX(cx):
    """the inclusive u32 sum up to the limit, in place; it wraps past 2^32, as the low 32 bits of the closed form do"""
    n = NMAX
    work_b = cx.size("adlhip_scan_typed_scratch_bytes", U32, n)
    vals = L.fill(cx.arena.take(n, I4, "values"), L.scan_sum_in)
    work, wb = cx.work(work_b)
    cx.call("adlhip_scan_typed", U32, SUM, 0, None, P(vals), P(vals), n, P(work), wb)
    L.check_equal(vals, L.scan_sum_out, n, "inclusive sum")
    cx.end("scan_typed u32 sum in place n=%d" % n)


@pytest.mark.parametrize("op", [MIN, MAX], ids=["min", "max"])
def test_scan_typed_u32_min_max_N31(cx, op):
    n = N31
    fin, fout = (L.scan_min_in(n), L.scan_min_out(n)) if op == MIN else (L.scan_max_in, L.scan_max_out)
    work_b = cx.size("adlhip_scan_typed_scratch_bytes", U32, n)
    vin = L.fill(cx.arena.take(n, I4, "values in", guarded=False), fin)
    out = cx.arena.take(n, I4, "out")
    work, wb = cx.work(work_b)
    cx.call("adlhip_scan_typed", U32, op, 0, None, P(vin), P(out), n, P(work), wb)
    L.check_equal(out, fout, n, "running min / max")
    L.check_equal(vin, fin, n, "the input afterwards")
    cx.end("scan_typed u32 op=%d n=%d" % (op, n))


def test_scan_typed_i64_exclusive_sum_with_init_NB8(cx):
    n, init = NB8, -(1 << 40) + 99
    work_b = cx.size("adlhip_scan_typed_scratch_bytes", I64, n)
    vin = L.fill(cx.arena.take(n, I8, "values in", guarded=False), L.scan_sum_in)
    out = cx.arena.take(n, I8, "out")
    work, wb = cx.work(work_b)
    cx.call("adlhip_scan_typed", I64, SUM, 1, cx.host(init, ctypes.c_int64), P(vin), P(out), n, P(work), wb)
    L.check_equal(out, L.scan_sum_exclusive_out(init), n, "exclusive sum")
    L.check_equal(vin, L.scan_sum_in, n, "the input afterwards")
    cx.end("scan_typed i64 exclusive n=%d" % n)


def test_scan_by_key_u32_ones_N31(cx):
    """the running count inside runs of 5, 5 and 6 keys"""
    n = N31
    r = L.Runs(n)
    work_b = cx.size("adlhip_scan_by_key_scratch_bytes", 4, U32, n)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), r.key)
    vin = cx.arena.take(n, I4, "values in", guarded=False)
    vin.fill_(1)
    out = cx.arena.take(n, I4, "out")
    work, wb = cx.work(work_b)
    cx.call("adlhip_scan_by_key", 4, P(kin), U32, SUM, 0, None, P(vin), P(out), n, P(work), wb)
    L.check_equal(out, r.count_so_far, n, "running count")
    L.check_equal(kin, r.key, n, "the keys afterwards")
    cx.end("scan_by_key n=%d" % n)


def test_exclusive_scan_u32_NMAX(cx):
    """Pprims::scan up to the limit; the total comes back to the host"""
    n = NMAX
    work_b = cx.size("adlhip_scan_scratch_bytes", n)
    src = L.fill(cx.arena.take(n, I4, "src", guarded=False), L.scan_sum_in)
    dst = cx.arena.take(n, I4, "dst")
    work, wb = cx.work(work_b)
    total = ctypes.c_uint32(0)
    cx.call("adlhip_exclusive_scan_u32", P(dst), P(src), P(work), wb, n, ctypes.cast(ctypes.pointer(total), ctypes.c_void_p))
    torch.cuda.synchronize()
    L.check_equal(dst, L.scan_sum_exclusive_out(0), n, "exclusive sum")
    last = torch.tensor([n - 1], dtype=I8)
    assert total.value == int(L.scan_sum_out(last)[0]) & L.M32
    cx.end("exclusive_scan_u32 n=%d" % n)


# ---------------------------------------------------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------------------------------------------------
def test_compact_flagged_NMAX(cx):
    """every third element, with its position"""
    n = NMAX
    c = L.flagged_count(n)
    work_b = cx.size("adlhip_compact_scratch_bytes", n)
    flags = L.fill(cx.arena.take(n, torch.uint8, "flags", guarded=False), L.flags_in)
    items = L.fill(cx.arena.take(n, I4, "items", guarded=False), L.Perm(n))
    out, index, num = cx.arena.take(n, I4, "items out"), cx.arena.take(n, I4, "index"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_compact_flagged", 4, P(items), P(flags), n, 0, P(out), P(index), P(num), P(work), wb)
    L.check_count(num, c, "number selected")
    L.check_equal(index, L.flagged_index_out, c, "positions")
    p = L.Perm(n)
    L.check_equal(out, lambda j: p(3 * j), c, "items")
    assert bool((out[c:c + (1 << 20)].view(torch.uint8) == SENTINEL).all()), "written behind the selected elements"
    L.check_equal(flags, L.flags_in, n, "the flags afterwards")
    L.check_equal(items, p, n, "the items afterwards")
    cx.end("compact_flagged n=%d" % n)


@pytest.mark.parametrize("partition", [0, 1], ids=["select", "partition"])
def test_compact_if_NMAX(cx, partition):
    """keys below T of a permutation: T selected, positions rising; a partition appends the rejected ones, positions rising"""
    n, T = NMAX, (1 << 31) + 777
    p = L.Perm(n)
    n_out = n if partition else T
    work_b = cx.size("adlhip_compact_scratch_bytes", n)
    kin = L.fill(cx.arena.take(n, I4, "keys in", guarded=False), p)
    kout, index, num = cx.arena.take(n, I4, "keys out"), cx.arena.take(n, I4, "index"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_compact_if_typed", U32, 0, cx.host(T, ctypes.c_uint32), P(kin), 0, None, n, partition, P(kout), None, P(index), P(num),
            P(work), wb)
    L.check_count(num, T, "number selected")
    L.check_range(index, n_out, n, "positions")
    L.check_rising(index[:T], None, T, "selected positions", everywhere=True)
    if partition:
        L.check_rising(index[T:], None, n - T, "rejected positions", everywhere=True)
    else:
        for t in (kout, index):
            assert bool((t[T:T + (1 << 20)].view(torch.uint8) == SENTINEL).all()), "written behind the selected elements"
    for lo, hi in L.chunks(n_out):
        keys = p(L.from_u32(index[lo:hi]))
        j = L.arange(lo, hi, index.device)
        assert bool(((keys < T) == (j < T)).all()), "an element on the wrong side in [%d, %d)" % (lo, hi)
        assert bool((L.from_u32(kout[lo:hi]) == keys).all()), "a key that is not the one at its position in [%d, %d)" % (lo, hi)
    L.check_equal(kin, p, n, "the input afterwards")
    cx.end("compact_if partition=%d n=%d" % (partition, n))


# ---------------------------------------------------------------------------------------------------------------------
# histograms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ktype,n,bins", [("u32", NMAX, 7), ("u32", NMAX, 50000), ("i64", NB8, 4096)],
                         ids=["u32-NMAX-7-bins", "u32-NMAX-50000-bins-sorted-path", "i64-NB8-4096-bins"])
def test_bincount(cx, ktype, n, bins):
    """7 and 4096 bins: counters in LDS; 50000 bins: the sorted path, whose work is a copy of the keys and their sort"""
    code, dt = L.KEY_TYPES[ktype], (I4 if ktype == "u32" else I8)
    fin, fout = L.bincount_in(n, bins), L.bincount_out(n, bins)
    work_b = cx.size("adlhip_histogram_scratch_bytes", code, n, bins, 0)
    kin = L.fill(cx.arena.take(n, dt, "keys in", guarded=False), fin)
    counts = cx.arena.take(bins, I4, "counts")
    work, wb = cx.work(work_b)
    cx.call("adlhip_bincount_typed", code, P(kin), n, bins, P(counts), P(work), wb)
    L.check_equal(counts, fout, bins, "counts")
    L.check_equal(kin, fin, n, "the input afterwards")
    cx.end("bincount %s n=%d bins=%d" % (ktype, n, bins))


@pytest.mark.parametrize("ktype,n,bins", [("u32", NMAX, 4096), ("u32", NMAX, 3), ("i64", NB8, 7)], ids=["u32-NMAX-4096", "u32-NMAX-3", "i64-NB8-7"])
def test_histogram_range(cx, ktype, n, bins):
    """edges over a permutation: a bin's count is its width; one repeated edge; keys outside the edges"""
    code, dt = L.KEY_TYPES[ktype], (I4 if ktype == "u32" else I8)
    p = L.Perm(n)
    work_b = cx.size("adlhip_histogram_scratch_bytes", code, n, bins, 1)
    kin = L.fill(cx.arena.take(n, dt, "keys in", guarded=False), p)
    edges = L.fill(cx.arena.take(bins + 1, dt, "edges", guarded=False), L.edges(n, bins))
    counts = cx.arena.take(bins, I4, "counts")
    work, wb = cx.work(work_b)
    cx.call("adlhip_histogram_range_typed", code, P(kin), n, P(edges), bins, 0, P(counts), P(work), wb)
    L.check_equal(counts, L.histogram_range_out(n, bins), bins, "counts")
    L.check_equal(kin, p, n, "the input afterwards")
    cx.end("histogram_range %s n=%d bins=%d" % (ktype, n, bins))


# ---------------------------------------------------------------------------------------------------------------------
# merge, set operations, search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb,vb", [(NMAX - (1 << 30) - 5, (1 << 30) + 5, 0), ((1 << 30) + 777, (1 << 30) + 12346, 4)],
                         ids=["NMAX-keys-index", "past-2p31-values-index"])
def test_merge_typed(cx, na, nb, vb):
    """ties within and across the inputs, unequal lengths; keys, positions in A || B and (second case) values"""
    m = L.Merge(na, nb)
    n = na + nb
    work_b = cx.size("adlhip_merge_scratch_bytes", U32, vb, na, nb)
    a = L.fill(cx.arena.take(na, I4, "a", guarded=False), L.merge_in)
    b = L.fill(cx.arena.take(nb, I4, "b", guarded=False), L.merge_in)
    va = vb_ = vout = None
    if vb:
        va = L.fill(cx.arena.take(na, I4, "values a", guarded=False), identity)
        vb_ = L.fill(cx.arena.take(nb, I4, "values b", guarded=False), lambda i: na + i)
        vout = cx.arena.take(n, I4, "values out")
    kout, index = cx.arena.take(n, I4, "keys out"), cx.arena.take(n, I4, "index")
    work, wb = cx.work(work_b)
    cx.call("adlhip_merge_typed", U32, ASC, P(a), P(va), na, P(b), P(vb_), nb, vb, P(kout), P(vout), P(index), P(work), wb)
    L.check_equal(kout, m.keys_out, n, "merged keys")
    L.check_equal(index, m.source, n, "positions")
    if vb:
        L.check_equal(vout, m.source, n, "values")
    L.check_equal(a, L.merge_in, na, "a afterwards")
    L.check_equal(b, L.merge_in, nb, "b afterwards")
    cx.end("merge na=%d nb=%d" % (na, nb))


SET_OPS = ["intersection", "union", "difference", "symmetric_difference"]


@pytest.mark.parametrize("op", range(4), ids=SET_OPS)
def test_set_op_typed_past_2p31(cx, op):
    """a = the even numbers, b = the multiples of 3, na + nb past 2^31, the keys past 2^31 too; keys, positions and the count"""
    na, nb = 1_200_000_011, 1_000_000_007
    assert na + nb > (1 << 31)
    s = L.SetOps(na, nb)
    name = SET_OPS[op]
    cap = na if name in ("intersection", "difference") else na + nb
    count = s.count(name)
    work_b = cx.size("adlhip_set_op_scratch_bytes", U32, 0, na, nb)
    a = L.fill(cx.arena.take(na, I4, "a", guarded=False), lambda i: 2 * i)
    b = L.fill(cx.arena.take(nb, I4, "b", guarded=False), lambda i: 3 * i)
    kout, index, num = cx.arena.take(cap, I4, "keys out"), cx.arena.take(cap, I4, "index"), cx.arena.take(4, I4, "count word")
    work, wb = cx.work(work_b)
    cx.call("adlhip_set_op_typed", U32, ASC, op, P(a), None, na, P(b), None, nb, 0, P(kout), None, P(index), P(num), P(work), wb)
    L.check_count(num, count, "size of the result")
    L.check_equal(kout, s.keys_out(name), count, name + " keys")
    L.check_equal(index, s.source(name), count, name + " positions")
    if count < cap:
        assert bool((kout[count:count + (1 << 20)].view(torch.uint8) == SENTINEL).all()), "written behind the result"
    L.check_equal(a, lambda i: 2 * i, na, "a afterwards")
    L.check_equal(b, lambda i: 3 * i, nb, "b afterwards")
    cx.end("set_op %s na=%d nb=%d" % (name, na, nb))


@pytest.mark.parametrize("side", [0, 1], ids=["left", "right"])
@pytest.mark.parametrize("m,n", [(N31, (1 << 20) + 3), ((1 << 20) + 3, N31)], ids=["N31-haystack", "N31-needles"])
def test_search_sorted(cx, m, n, side):
    """every multiple of 3 twice; the needles sweep the haystack's range and a little beyond"""
    top = 3 * (m >> 1) + 50
    needle = (lambda i: (i * 2999) % top) if n < m else (lambda i: i % top)
    want = L.search_left(m) if side == 0 else L.search_right(m)
    hay = L.fill(cx.arena.take(m, I4, "haystack", guarded=False), L.haystack)
    needles = L.fill(cx.arena.take(n, I4, "needles", guarded=False), needle)
    pos = cx.arena.take(n, I4, "positions")
    cx.call("adlhip_search_sorted_typed", U32, ASC, side, P(hay), m, P(needles), n, P(pos))
    L.check_equal(pos, lambda i: want(needle(i)), n, "positions")
    L.check_equal(hay, L.haystack, m, "the haystack afterwards")
    L.check_equal(needles, needle, n, "the needles afterwards")
    cx.end("search m=%d n=%d side=%d" % (m, n, side))


# ---------------------------------------------------------------------------------------------------------------------
# scratch sizes
# ---------------------------------------------------------------------------------------------------------------------
def scratch_queries():
    """label -> (function, the arguments in front of the size_t outputs as a function of n, the number of outputs)"""
    ceil = lambda n, d: -(-n // d)   # noqa: E731
    return {
        "radix_sort u32": ("adlhip_radix_sort_scratch_bytes", lambda n: (0, n), 2),
        "radix_sort kv32": ("adlhip_radix_sort_scratch_bytes", lambda n: (1, n), 2),
        "radix_sort u64": ("adlhip_radix_sort_scratch_bytes", lambda n: (2, n), 2),
        "radix_sort soa32": ("adlhip_radix_sort_scratch_bytes", lambda n: (3, n), 2),
        "radix_sort_for lean": ("adlhip_radix_sort_scratch_bytes_for", lambda n: (0, n, 32, 2), 2),
        "radix_sort_soa 8/16": ("adlhip_radix_sort_soa_scratch_bytes", lambda n: (8, 16, n, 64), 3),
        "sort_typed keys": ("adlhip_sort_typed_scratch_bytes", lambda n: (F32, 0, 0, n), 3),
        "sort_typed pairs": ("adlhip_sort_typed_scratch_bytes", lambda n: (F64, 1, 16, n), 3),
        "sort_typed argsort": ("adlhip_sort_typed_scratch_bytes", lambda n: (I32, 2, 0, n), 3),
        "topk": ("adlhip_topk_scratch_bytes", lambda n: (F32, n, 1000), 1),
        "topk_rows": ("adlhip_topk_rows_scratch_bytes", lambda n: (F32, 3, n, 1000), 1),
        # rows * cols is what the limit bounds: the largest whole number of rows at N31 and NMAX, one row more than fits at NMAX + 1
        "sort_rows row kernel": ("adlhip_sort_rows_scratch_bytes", lambda n: (I32, n // 32 if n <= NMAX else ceil(n, 32), 32), 1),
        "sort_rows flat": ("adlhip_sort_rows_scratch_bytes", lambda n: (I32, n // 4099 if n <= NMAX else ceil(n, 4099), 4099), 1),
        "sort_segments plan": ("adlhip_sort_segments_scratch_bytes", lambda n: (I32, n, n // 512, 4096), 1),
        "sort_segments flat": ("adlhip_sort_segments_scratch_bytes", lambda n: (I32, n, n // 512, 0), 1),
        "run_length_encode": ("adlhip_run_length_encode_scratch_bytes", lambda n: (4, n), 1),
        "unique": ("adlhip_unique_scratch_bytes", lambda n: (I64, n, 1), 1),
        "reduce_runs": ("adlhip_reduce_runs_scratch_bytes", lambda n: (8, F64, n), 1),
        "reduce_by_key": ("adlhip_reduce_by_key_scratch_bytes", lambda n: (I64, F64, n), 1),
        "scan_typed": ("adlhip_scan_typed_scratch_bytes", lambda n: (F64, n), 1),
        "scan_by_key": ("adlhip_scan_by_key_scratch_bytes", lambda n: (8, F64, n), 1),
        "compact": ("adlhip_compact_scratch_bytes", lambda n: (n,), 1),
        "histogram lds": ("adlhip_histogram_scratch_bytes", lambda n: (U32, n, 4096, 1), 1),
        "histogram sorted": ("adlhip_histogram_scratch_bytes", lambda n: (U32, n, 50000, 0), 1),
        "merge": ("adlhip_merge_scratch_bytes", lambda n: (U32, 8, n - n // 3, n // 3), 1),
        "set_op": ("adlhip_set_op_scratch_bytes", lambda n: (U32, 8, n - n // 3, n // 3), 1),
        "scan": ("adlhip_scan_scratch_bytes", lambda n: (n,), 1),
    }


@pytest.mark.parametrize("query", list(scratch_queries()))
def test_scratch_sizes_at_the_top_of_the_range(cx, query):
    """every *_scratch_bytes at N31 and NMAX: succeeds, reports no less than at half the size, and refuses NMAX + 1 (a host check: nothing
    is launched)"""
    name, args, outs = scratch_queries()[query]
    for n in (N31, NMAX):
        full = cx.size(name, *args(n), outs=outs)
        half = cx.size(name, *args(n // 2), outs=outs)
        full, half = (full, half) if outs > 1 else ([full], [half])
        assert all(f >= h for f, h in zip(full, half)), (query, n, full, half)
        assert all(f < (1 << 40) for f in full), (query, n, full)
    over = args(NMAX + 1)
    vals = [ctypes.c_size_t(0) for _ in range(outs)]
    assert cx.refused(name, *over, *[ctypes.byref(v) for v in vals]), query + " accepts more than the limit"
    cx.end("scratch sizes " + query)


def test_the_verifier_on_the_device_names_an_element_past_2p31(cx):
    """the planted errors of tests/test_large_n_forms.py once more where the GPU cases look: one flipped bit and one repeated index behind
    element 2^31 of a device tensor"""
    n, at = N31, (1 << 31) + 4321
    t = L.fill(cx.arena.take(n, I4, "values", guarded=False), identity)
    L.check_equal(t, identity, n, "values")
    L.check_rising(t, None, n, "values", everywhere=True)
    t[at] ^= 1 << 9
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(t, identity, n, "values")
    assert e.value.index == at and e.value.got ^ e.value.want == 1 << 9
    t[at] = t[at - 1]
    with pytest.raises(L.Mismatch) as e:
        L.check_rising(t, None, n, "values", everywhere=True)
    assert e.value.index == at
    cx.end("the verifier past 2^31")
