"""The typed primitives on the sort's fallback configurations (tests/typed_fallbacks.py has the configurations, the sizes and the rules
that read a profile's launch labels; tests/typed_shapes.py the keys and the expected order).

Nine typed entry points run the unsigned radix sort beneath them; their own suites run that sort almost only in the configuration an
unpartitioned MI355X picks by itself.  Here every one of them runs under five configurations -- the default as the control, "sort.rank"
= 0 (the LDS-order self-test failed), "debug.resident_wgs" = 120 (a partition that cannot keep 256 workgroups resident), "sort.algo" = 0
(the per-digit look-back passes) and "sort.algo" = 1 with "sort.digit_bits" = 4 (the reference's eight 4-bit passes and the copy back
behind an odd pass count) -- on value-shaped keys: the high dwords of float64 under one top byte, int64 ids that share one high dword,
30 % of the keys one NaN pattern, an index half that is all distinct.

Every call checks the whole contract:
  1. the outputs are bit-exact against numpy (indices, counts and the count word included); the expected results are computed once per
     (primitive, case, n, order) and shared by the five configurations -- never taken from another GPU run;
  2. the input is bit-identical afterwards;
  3. every output lies between guard regions that are unchanged, the work buffer has exactly the queried size -- queried after the
     knobs are set --, holds garbage on entry and has guards of its own;
  4. adlhip_fault_check is clean and "debug.idle_dirty" reads 0;
  5. the launch labels show that the configuration reached the inner sort (typed_fallbacks.check_labels).
One handle serves the whole module, so calls of different primitives, sizes and configurations follow each other on it with no
synchronisation beyond what reading the results needs.

The control.  A sort in the mid-size range may be sent down the per-digit passes by the reports of earlier sorts on the handle
(adlhip.hip choose_mid_form), and every case here but uniform bits raises such a report.  So the `default` configuration asserts per
call what no report can change (the large forms show; a mid-size sort shows the mid-size form or the 8-bit passes), and per rung, on
uniform bits and a handle of its own that has sorted nothing else, that the size class shows in the names: if a threshold moves and
a rung stops telling the forms apart, that fails.

Knobs changed after the scratch was sized.  include/adlhip.h promises for the typed sorts, unique and reduce by key that "a sort that
refuses (knobs changed since the scratch was sized) fails the call with the sort's message".  No test of that is here, for any entry
point: NO configuration asks for more scratch than the default.  The typed queries take the larger of the per-digit paths' tables, the
mid-size form's layout (4 MiB of slabs at least) and, above 16384 elements, the large sort's slabs (three times the data); the
look-back passes' status rows -- the only part that grows with "sort.digit_bits" and "sort.tile" -- stay below both at every n the
large sort takes (up to 260 Mi elements), and "sort.algo", "sort.rank" and "debug.resident_wgs" enter no layout.
test_no_configuration_asks_for_more_scratch_than_the_default asserts exactly that on the host, for every entry point, size and
configuration used here and for every "sort.tile": the day one of them asks for more, it fails and the refusal
can be tested.  (The in-place entry points are covered by test_a_refused_typed_sort_leaves_keys_and_values_as_they_were, which hands the
base sort less than the typed query.)
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in test_gpu_typed_sort.py)

import typed_fallbacks as tf
from oclradixsort_amd import Buffer, DeviceUtils, _lib
from test_gpu_call_sequences import STABLE_KV, assert_idle
from test_gpu_parity import LARGE_PAIRS
from test_gpu_reduce import SUM, by_key_oracle
from test_gpu_sort_rows import Case as RowsCase, Framed
from test_gpu_sort_segments import Case as SegmentsCase
from test_gpu_typed_sort import random_bits
from test_gpu_unique import unique_oracle
from typed_fallbacks import Sort
from typed_shapes import ASC, BY_NAME, DESC, expected_perm, shape

pytestmark = pytest.mark.gpu

ORDERS = (ASC, DESC)
F64 = BY_NAME["f64"][1]
GARBAGE, UNWRITTEN = 0xa7, 0xcd
ROWS_FLAT = SEGMENTS_FLAT = TOPK_ROWS_LOOP = 0
SEGMENTS_KERNEL = 1
LOCAL, GLOBAL = 0, 1
# the label sets of the large stable pair sort, as the suite states them elsewhere (the finish is missing where the net ran)
assert tf.STABLE_PAIRS | {"segment_sort_wave_e64"} == LARGE_PAIRS == STABLE_KV
KNOBS_OF_THE_PATHS = {"sort.rows_algo": -1, "sort.segments_algo": -1, "topk.rows_algo": -1, "topk.algo": -1, "unique.algo": -1}


# ---------------------------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------------------------
def lib_err():
    e = _lib.load().adlhip_last_error()
    return e.decode() if e else ""


def restore(d):
    for knob, back in tf.RESTORE.items():
        d.setParam(knob, d.getParam(back) if isinstance(back, str) else back)
    for knob, back in KNOBS_OF_THE_PATHS.items():
        d.setParam(knob, back)


@pytest.fixture(scope="module")
def dev():
    d = DeviceUtils.allocate()
    yield d
    restore(d)
    d.toggleProfiling(False)
    DeviceUtils.deallocate(d)


class Store:
    """what the configurations share: the expected results (host) and the inputs that stay on the device"""

    def __init__(self, dev):
        self.dev = dev
        self.once = tf.Once()
        self.device = {}

    def bits(self, name, case, n):
        return self.once.get(("bits", name, case, n), lambda: shape(name, case, n, tf.SEED))

    def perm(self, name, case, n, order):
        return self.once.get(("perm", name, case, n, order), lambda: expected_perm(self.bits(name, case, n), name, order))

    def expected(self, what, bits, order, make):
        """make() once per (primitive, keys, order) for the keys bits() handed out (they stay alive here, so their id names them);
        keys of a control are not kept"""
        if any(bits is held for key, held in self.once.have.items() if key[0] == "bits"):
            return self.once.get((what, id(bits), order), make)
        return make()

    def on_device(self, key, make):
        if key not in self.device:
            self.device[key] = make()
        return self.device[key]

    def input(self, name, case, n):
        return self.on_device(("input", name, case, n), lambda: Framed(self.dev, payload=self.bits(name, case, n), front=48, seed=5))

    def release(self):
        for held in self.device.values():
            held.release()
        self.device.clear()


@pytest.fixture(scope="module")
def store(dev):
    s = Store(dev)
    yield s
    s.release()


@contextlib.contextmanager
def configured(d, config, **paths):
    """the configuration's knobs (and the knob that forces a primitive's path) for the block, put back whatever happens; per-launch
    profiling is on inside"""
    try:
        for knob, value in tf.KNOBS_OF[config]:
            d.setParam(knob, value)
        for knob, value in paths.items():
            d.setParam(knob.replace("__", "."), value)
        d.toggleProfiling(True)
        d.profile(reset=True)
        yield
    finally:
        d.toggleProfiling(False)
        restore(d)


class Work:
    """exactly `need` bytes of garbage between two guard regions"""

    GUARD = 256

    def __init__(self, d, need, seed=8):
        self.dev, self.need = d, int(need)
        rng = np.random.default_rng(seed)
        self.front, self.back = (rng.integers(0, 256, size=self.GUARD, dtype=np.uint8) for _ in range(2))
        self.buf = Buffer(d, 2 * self.GUARD + self.need, np.uint8)
        self.buf.write(self.front)
        if self.need:
            assert _lib.load().adlhip_memset(d._h, self.ptr(), GARBAGE, self.need) == 0, lib_err()
        self.buf.write(self.back, dstOffsetNElems=self.GUARD + self.need)

    def ptr(self):
        return ctypes.c_void_p(self.buf.m_ptr + self.GUARD)

    def check(self):
        front, back = np.empty(self.GUARD, np.uint8), np.empty(self.GUARD, np.uint8)
        self.buf.read(front)
        self.buf.read(back, srcOffsetNElems=self.GUARD + self.need)
        DeviceUtils.waitForCompletion(self.dev)
        assert np.array_equal(front, self.front), "bytes in front of the work buffer were written"
        assert np.array_equal(back, self.back), "bytes behind the work buffer were written"

    def release(self):
        self.buf.release()


def query(fn, d, *args):
    wb = ctypes.c_size_t()
    assert fn(d._h, *args, ctypes.byref(wb)) == 0, lib_err()
    return wb.value


def typed_query(d, kt, mode, vb, n):
    tk, tv, wb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = _lib.load().adlhip_sort_typed_scratch_bytes(d._h, kt, mode, vb, n, ctypes.byref(tk), ctypes.byref(tv), ctypes.byref(wb))
    assert rc == 0, lib_err()
    return tk.value, tv.value, wb.value


def net_stats(d):
    return d.getParam("stat.net_runs"), d.getParam("stat.net_counting")


class Call:
    """One call of an entry point: its buffers, and after it every check that does not depend on the primitive -- the guards of the work
    buffer, the inputs, the fault word, the idle state, the labels.  The outputs are read through Framed.read, which asserts their
    guards."""

    def __init__(self, d, judge, sorts):
        self.dev, self.judge, self.sorts = d, judge, sorts
        self.mine, self.inputs, self.work = [], [], None
        self.before = net_stats(d)

    def reads(self, framed):
        """an input that outlives the call (the store's or the control's): must be unchanged afterwards"""
        self.inputs.append(framed)

    def inout(self, payload, seed=6):
        f = Framed(self.dev, payload=payload, seed=seed)
        self.mine.append(f)
        return f

    def out(self, nbytes, seed=7):
        f = Framed(self.dev, nbytes=int(nbytes), fill=UNWRITTEN, seed=seed)
        self.mine.append(f)
        return f

    def scratch(self, need):
        self.work = Work(self.dev, need)
        return self.work

    def done(self, rc, what):
        """after the outputs have been read"""
        assert rc == 0, "%s: %s" % (what, lib_err())
        self.work.check()
        for f in self.inputs:
            assert f.unchanged(), what + ": an input was changed"
        self.dev.checkFault()
        assert_idle(self.dev, what)
        after = net_stats(self.dev)
        labels = set(self.dev.profile(reset=True))
        self.judge(labels, self.sorts, (after[0] - self.before[0], after[1] - self.before[1]))

    def release(self):
        for f in self.mine:
            f.release()
        if self.work is not None:
            self.work.release()


def judge_of(config):
    return lambda labels, sorts, net_delta: tf.check_labels(config, labels, sorts, net_delta)


def control_judge(labels, sorts, net_delta):
    tf.check_control(labels, sorts)


@contextlib.contextmanager
def control_handle(config):
    """default only: a handle of its own for the rungs' controls on uniform bits (None otherwise)"""
    if config != "default":
        yield None
        return
    d = DeviceUtils.allocate()
    try:
        d.toggleProfiling(True)
        yield d
    finally:
        d.toggleProfiling(False)
        DeviceUtils.deallocate(d)


def uniform(name, n):
    return random_bits(BY_NAME[name][3], n, 900 + BY_NAME[name][1])


def positions(n, dtype):
    """values that are the positions: stability shows in them"""
    return np.arange(n, dtype=dtype)


def keys_kind(bits):
    return "keys32" if bits.dtype.itemsize == 4 else "keys64"


def unwritten(arr):
    return bool((arr.view(np.uint8) == UNWRITTEN).all())


# ---------------------------------------------------------------------------------------------
# one call of every entry point
# ---------------------------------------------------------------------------------------------
def run_sort_keys(d, judge, name, order, bits, want):
    n, kt = bits.size, BY_NAME[name][1]
    what = "sort_keys %s order %d n %d" % (name, order, n)
    c = Call(d, judge, [Sort(keys_kind(bits), n)])
    try:
        tk, _, wb = typed_query(d, kt, 0, 0, n)
        assert tk >= bits.nbytes
        k = c.inout(bits)
        t = c.out((bits.nbytes + 15) // 16 * 16)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_sort_keys_typed(d._h, kt, order, k.ptr(), t.ptr(), w.ptr(), wb, n)
        got = k.read(bits.dtype)
        t.read()
        c.done(rc, what)
        assert np.array_equal(got, want), what + ": keys differ"
    finally:
        c.release()


def run_sort_pairs(d, judge, name, order, bits, perm):
    n, kt = bits.size, BY_NAME[name][1]
    vals = positions(n, bits.dtype)   # 4-byte values beside 4-byte keys, 8-byte values beside 8-byte keys
    vb = vals.dtype.itemsize
    what = "sort_pairs %s order %d n %d" % (name, order, n)
    c = Call(d, judge, [Sort("pairs", n)] * (bits.dtype.itemsize // 4))
    try:
        tk, tv, wb = typed_query(d, kt, 1, vb, n)
        assert tv >= vals.nbytes and (tk == 0 or tk >= bits.nbytes)
        k, v = c.inout(bits, seed=6), c.inout(vals, seed=9)
        tkb, tvb = c.out((bits.nbytes + 15) // 16 * 16, seed=10), c.out((vals.nbytes + 15) // 16 * 16, seed=11)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_sort_pairs_typed(d._h, kt, order, k.ptr(), v.ptr(), vb, tkb.ptr() if tk else None, tvb.ptr(), w.ptr(), wb, n)
        got_k, got_v = k.read(bits.dtype), v.read(vals.dtype)
        tkb.read()
        tvb.read()
        c.done(rc, what)
        assert np.array_equal(got_k, bits[perm]), what + ": keys differ"
        assert np.array_equal(got_v, perm.astype(vals.dtype)), what + ": values differ (equal keys must keep their input order)"
    finally:
        c.release()


def run_argsort(d, judge, name, order, bits, inp, perm):
    n, kt = bits.size, BY_NAME[name][1]
    what = "argsort %s order %d n %d" % (name, order, n)
    c = Call(d, judge, [Sort("pairs", n)] * (bits.dtype.itemsize // 4))
    try:
        wb = typed_query(d, kt, 2, 0, n)[2]
        c.reads(inp)
        ko, io = c.out(bits.nbytes, seed=6), c.out(4 * n, seed=7)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_argsort_typed(d._h, kt, order, inp.ptr(), ko.ptr(), io.ptr(), w.ptr(), wb, n)
        got_i, got_k = io.read(np.uint32), ko.read(bits.dtype)
        c.done(rc, what)
        assert np.array_equal(got_i, perm.astype(np.uint32)), what + ": indices differ"
        assert np.array_equal(got_k, bits[perm]), what + ": keys differ"
    finally:
        c.release()


def topk_sorts(select, width, n, k):
    if select:   # the k positions as u32 keys, then the stable pair sort of the k (key, position) pairs
        return [Sort("positions", k)] + [Sort("pairs", k)] * (width // 4)
    return [Sort("pairs", n)] * (width // 4)


def run_topk(d, judge, name, order, bits, inp, perm, k, select):
    n, kt, w_item = bits.size, BY_NAME[name][1], bits.dtype.itemsize
    what = "topk %s order %d n %d k %d %s" % (name, order, n, k, "selection" if select else "full argsort")
    c = Call(d, judge, topk_sorts(select, w_item, n, k))
    try:
        wb = query(_lib.load().adlhip_topk_scratch_bytes, d, kt, n, k)
        c.reads(inp)
        ko, io = c.out(k * w_item, seed=6), c.out(4 * k, seed=7)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_topk_typed(d._h, kt, order, inp.ptr(), n, k, ko.ptr(), io.ptr(), w.ptr(), wb)
        got_i, got_k = io.read(np.uint32), ko.read(bits.dtype)
        c.done(rc, what)
        assert np.array_equal(got_i, perm[:k].astype(np.uint32)), what + ": indices differ"
        assert np.array_equal(got_k, bits[perm[:k]]), what + ": keys differ"
    finally:
        c.release()


def run_topk_rows(d, judge, name, order, flat, inp, perms, rows, cols, stride, k, select):
    kt, w_item = BY_NAME[name][1], flat.dtype.itemsize
    what = "topk_rows %s order %d rows %d cols %d stride %d k %d %s" % (name, order, rows, cols, stride, k, "selection" if select else "full argsort")
    c = Call(d, judge, topk_sorts(select, w_item, cols, k))
    try:
        wb = query(_lib.load().adlhip_topk_rows_scratch_bytes, d, kt, rows, cols, k)
        c.reads(inp)
        ko, io = c.out(rows * k * w_item, seed=6), c.out(4 * rows * k, seed=7)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_topk_rows_typed(d._h, kt, order, inp.ptr(), rows, cols, stride, k, ko.ptr(), io.ptr(), w.ptr(), wb)
        got_i, got_k = io.read(np.uint32).reshape(rows, k), ko.read(flat.dtype).reshape(rows, k)
        c.done(rc, what)
        for r in range(rows):
            row = flat[r * stride:r * stride + cols]
            assert np.array_equal(got_i[r], perms[r][:k].astype(np.uint32)), "%s: columns differ in row %d" % (what, r)
            assert np.array_equal(got_k[r], row[perms[r][:k]]), "%s: keys differ in row %d" % (what, r)
    finally:
        c.release()


def count_word(c):
    return c.out(16, seed=12)   # the count word is its bytes 4 .. 7


def read_count(cw, what):
    word = cw.read(np.uint32)
    assert word[0] == word[2] == word[3] == 0xcdcdcdcd, what + ": bytes beside the count word were written"
    return int(word[1])


def run_unique(d, judge, name, order, bits, inp, exp, index_path):
    """index_path: "unique.algo" = 1 is in force and first_index and inverse are asked; otherwise counts and offsets only (the keys path)"""
    n, kt = bits.size, BY_NAME[name][1]
    what = "unique %s order %d n %d %s" % (name, order, n, "index path" if index_path else "keys path")
    width = bits.dtype.itemsize
    c = Call(d, judge, [Sort("pairs", n)] * (width // 4) if index_path else [Sort(keys_kind(bits), n)])
    try:
        wb = query(_lib.load().adlhip_unique_scratch_bytes, d, kt, n, 1 if index_path else 0)
        c.reads(inp)
        outs = {"unique": c.out(bits.nbytes, seed=20), "counts": c.out(4 * n, seed=21), "offsets": c.out(4 * (n + 1), seed=22)}
        if index_path:
            outs["first"], outs["inverse"] = c.out(4 * n, seed=23), c.out(4 * n, seed=24)
        cw = count_word(c)
        w = c.scratch(wb)
        p = {k: f.ptr() for k, f in outs.items()}
        rc = _lib.load().adlhip_unique_typed(d._h, kt, order, inp.ptr(), n, p["unique"], p["counts"], p["offsets"], p.get("first"),
                                             p.get("inverse"), cw.ptr(4), w.ptr(), wb)
        got = {k: f.read(bits.dtype if k == "unique" else np.uint32) for k, f in outs.items()}
        r = read_count(cw, what)
        c.done(rc, what)
        assert r == exp["unique"].size, "%s: the count word is %d, expected %d" % (what, r, exp["unique"].size)
        for k, g in got.items():
            m = n if k == "inverse" else r + (1 if k == "offsets" else 0)
            assert np.array_equal(g[:m], exp[k]), "%s: %s differs" % (what, k)
            assert unwritten(g[m:]), "%s: %s was written at index %d or beyond" % (what, k, m)
    finally:
        c.release()


def run_reduce_by_key(d, judge, name, order, bits, inp, vals, vin, exp):
    n, kt = bits.size, BY_NAME[name][1]
    what = "reduce_by_key %s order %d n %d" % (name, order, n)
    c = Call(d, judge, [Sort("pairs", n)] * (bits.dtype.itemsize // 4))
    try:
        wb = query(_lib.load().adlhip_reduce_by_key_scratch_bytes, d, kt, F64, n)
        c.reads(inp)
        c.reads(vin)
        outs = {"unique": c.out(bits.nbytes, seed=20), "reduced": c.out(8 * n, seed=21), "counts": c.out(4 * n, seed=22),
                "offsets": c.out(4 * (n + 1), seed=23)}
        cw = count_word(c)
        w = c.scratch(wb)
        rc = _lib.load().adlhip_reduce_by_key_typed(d._h, kt, order, inp.ptr(), F64, SUM, vin.ptr(), n, outs["unique"].ptr(), outs["reduced"].ptr(),
                                                    outs["counts"].ptr(), outs["offsets"].ptr(), cw.ptr(4), w.ptr(), wb)
        dtypes = {"unique": bits.dtype, "reduced": np.uint64}
        got = {k: f.read(dtypes.get(k, np.uint32)) for k, f in outs.items()}
        r = read_count(cw, what)
        c.done(rc, what)
        assert r == exp["unique"].size, "%s: the count word is %d, expected %d" % (what, r, exp["unique"].size)
        for k, g in got.items():
            m = r + (1 if k == "offsets" else 0)
            assert np.array_equal(g[:m], exp[k]), "%s: %s differs" % (what, k)
            assert unwritten(g[m:]), "%s: %s was written at index %d or beyond" % (what, k, m)
    finally:
        c.release()


def judged_case_run(d, judge, sorts, run):
    """a call through the Case classes of test_gpu_sort_rows / test_gpu_sort_segments, which check outputs, guards, input, work buffer,
    fault word and idle state themselves; here the labels"""
    before = net_stats(d)
    d.profile(reset=True)
    run()
    after = net_stats(d)
    judge(set(d.profile(reset=True)), sorts, (after[0] - before[0], after[1] - before[1]))


# ---------------------------------------------------------------------------------------------
# the matrix: (entry point, configuration)
# ---------------------------------------------------------------------------------------------
def entry_sort_keys(d, store, config, control):
    if control is not None:
        for name, n in (("f32", tf.KEY_RUNGS[4][0]), ("f32", tf.KEY_RUNGS[4][1]), ("f64", tf.KEY_RUNGS[8][0]), ("f64", tf.KEY_RUNGS[8][1])):
            x = uniform(name, n)
            run_sort_keys(control, control_judge, name, ASC, x, x[expected_perm(x, name, ASC)])
    with configured(d, config):
        for name, case in tf.CASES:
            for n in tf.KEY_RUNGS[BY_NAME[name][3]().itemsize]:
                bits = store.bits(name, case, n)
                for order in ORDERS:
                    run_sort_keys(d, judge_of(config), name, order, bits, bits[store.perm(name, case, n, order)])


def pair_controls(control, run):
    """the rungs' controls of an entry point that sorts pairs: 8-byte keys, so both dwords' sorts must show their size class"""
    if control is not None:
        for n in tf.PAIR_RUNGS:
            x = uniform("i64", n)
            inp = Framed(control, payload=x, front=48, seed=5)
            try:
                run(control, control_judge, "i64", ASC, x, inp, expected_perm(x, "i64", ASC))
            finally:
                inp.release()


def every_case(d, store, config, run, **paths):
    with configured(d, config, **paths):
        for name, case in tf.CASES:
            for n in tf.PAIR_RUNGS:
                bits, inp = store.bits(name, case, n), store.input(name, case, n)
                for order in ORDERS:
                    run(d, judge_of(config), name, order, bits, inp, store.perm(name, case, n, order))


def entry_sort_pairs(d, store, config, control):
    def run(dd, judge, name, order, bits, inp, perm):
        run_sort_pairs(dd, judge, name, order, bits, perm)
    pair_controls(control, run)
    every_case(d, store, config, run)


def entry_argsort(d, store, config, control):
    pair_controls(control, run_argsort)
    every_case(d, store, config, run_argsort)


def entry_topk(select):
    def entry(d, store, config, control):
        def run(dd, judge, name, order, bits, inp, perm):
            for k in tf.topk_ks(bits.size)[1 if dd is control else 0:]:   # (the control: the k on the rung)
                run_topk(dd, judge, name, order, bits, inp, perm, k, select)
        if control is not None:
            control.setParam("topk.algo", 1 if select else 0)
        pair_controls(control, run)
        every_case(d, store, config, run, topk__algo=1 if select else 0)
    return entry


def entry_topk_rows(d, store, config, control):
    """the per-row loop ("topk.rows_algo" = 0); "topk.algo" stays -1, so the first k of topk_ks takes the selection and the second the
    full argsort, row by row.  The strided shapes start their rows off the 16-byte grid: the selection then stages the row."""
    def run(dd, judge, name, order, flat, inp, perms, shp, forced=None):
        rows, cols, stride = shp
        for k, select in zip(tf.topk_ks(cols), (True, False)) if forced is None else [forced]:
            run_topk_rows(dd, judge, name, order, flat, inp, perms, rows, cols, stride, k, select)

    def row_perms(flat, name, order, shp):
        rows, cols, stride = shp
        return [expected_perm(flat[r * stride:r * stride + cols], name, order) for r in range(rows)]

    if control is not None:
        control.setParam("topk.rows_algo", TOPK_ROWS_LOOP)
        # the k on the rung through either path of the row's top-k, forced; every full argsort first: the selection's sort of
        # positions leaves reports behind that would decide for the sorts after it
        for select in (False, True):
            control.setParam("topk.algo", 1 if select else 0)
            for shp in tf.TOPK_ROW_SHAPES:
                x = uniform("i64", (shp[0] - 1) * shp[2] + shp[1])
                inp = Framed(control, payload=x, front=48, seed=5)
                try:
                    run(control, control_judge, "i64", ASC, x, inp, row_perms(x, "i64", ASC, shp), shp, forced=(tf.topk_ks(shp[1])[1], select))
                finally:
                    inp.release()
    with configured(d, config, topk__rows_algo=TOPK_ROWS_LOOP):
        for name, case in tf.CASES:
            for shp in tf.TOPK_ROW_SHAPES:
                total = (shp[0] - 1) * shp[2] + shp[1]
                flat, inp = store.bits(name, case, total), store.input(name, case, total)
                for order in ORDERS:
                    perms = store.once.get(("topk_rows", name, case, shp, order), lambda: row_perms(flat, name, order, shp))
                    run(d, judge_of(config), name, order, flat, inp, perms, shp)


def entry_sort_rows(d, store, config, control):
    """the flat path ("sort.rows_algo" = 0): the argsort of all keys, then adlhip_radix_sort_soa32 on the bits of the row id"""
    def sorts(name, n):
        return [Sort("pairs", n)] * (BY_NAME[name][3]().itemsize // 4) + [Sort("soa", n)]

    if control is not None:
        control.setParam("sort.rows_algo", ROWS_FLAT)
        for rows, cols, stride in tf.ROW_SHAPES:
            c = RowsCase(control, "i64", uniform("i64", (rows - 1) * stride + cols), rows, cols, stride)
            try:
                judged_case_run(control, control_judge, sorts("i64", rows * cols), lambda: c.run(ASC))
            finally:
                c.release()
    with configured(d, config, sort__rows_algo=ROWS_FLAT):
        for name, case in tf.CASES:
            for rows, cols, stride in tf.ROW_SHAPES:
                total = (rows - 1) * stride + cols
                c = store.on_device(("rows", name, case, rows), lambda: RowsCase(d, name, store.bits(name, case, total), rows, cols, stride))
                for order in ORDERS:
                    judged_case_run(d, judge_of(config), sorts(name, rows * cols), lambda: c.run(order))


def entry_sort_segments(d, store, config, control):
    """the flat path ("sort.segments_algo" = 0): 301 segments whose lengths vary, empty ones among them; local and global indices"""
    def sorts(name, n):
        return [Sort("pairs", n)] * (BY_NAME[name][3]().itemsize // 4) + [Sort("soa", n)]

    if control is not None:
        control.setParam("sort.segments_algo", SEGMENTS_FLAT)
        for n in tf.PAIR_RUNGS:
            c = SegmentsCase(control, "i64", uniform("i64", n), tf.segment_lengths(n, 301, 1))
            try:
                judged_case_run(control, control_judge, sorts("i64", n), lambda: c.run(ASC))
            finally:
                c.release()
    with configured(d, config, sort__segments_algo=SEGMENTS_FLAT):
        for name, case in tf.CASES:
            for n in tf.PAIR_RUNGS:
                c = store.on_device(("segments", name, case, n),
                                    lambda: SegmentsCase(d, name, store.bits(name, case, n), tf.segment_lengths(n, 301, 1)))
                for order in ORDERS:
                    judged_case_run(d, judge_of(config), sorts(name, n), lambda: c.run(order, base=GLOBAL if order == DESC else LOCAL))


def entry_sort_segments_plan(d, store, config, control):
    """the segment kernel ("sort.segments_algo" = 1), whose plan sorts 20011 (class, segment id) pairs stably on 4 bits with
    adlhip_radix_sort_soa32.  That sort has no size classes -- on fewer than 16 bits it runs the per-digit passes whatever its size --
    so the default needs no control of a rung here; every other configuration must show in its labels."""
    n = tf.PAIR_RUNGS[1]
    with configured(d, config, sort__segments_algo=SEGMENTS_KERNEL):
        for name, case in tf.CASES:
            c = store.on_device(("plan", name, case), lambda: SegmentsCase(d, name, store.bits(name, case, n),
                                                                           tf.segment_lengths(n, tf.PLAN_SEGMENTS, 2, longest=4096)))
            for order in ORDERS:
                judged_case_run(d, judge_of(config), [Sort("soa", tf.PLAN_SEGMENTS)], lambda: c.run(order, base=GLOBAL if order == DESC else LOCAL))


def entry_unique_keys(d, store, config, control):
    """"unique.algo" = -1 with counts and offsets only: the keys path, a copy of the keys through adlhip_sort_keys_typed's sort -- whole
    keys, so the sizes are that entry point's"""
    def run(dd, judge, name, order, bits):
        exp = store.expected("unique", bits, order, lambda: unique_oracle(bits, name, order))
        inp = Framed(dd, payload=bits, front=48, seed=5)
        try:
            run_unique(dd, judge, name, order, bits, inp, exp, False)
        finally:
            inp.release()

    if control is not None:
        for name, n in (("f32", tf.KEY_RUNGS[4][0]), ("f32", tf.KEY_RUNGS[4][1]), ("f64", tf.KEY_RUNGS[8][0]), ("f64", tf.KEY_RUNGS[8][1])):
            run(control, control_judge, name, ASC, uniform(name, n))
    with configured(d, config):
        for name, case in tf.CASES:
            for n in tf.KEY_RUNGS[BY_NAME[name][3]().itemsize]:
                for order in ORDERS:
                    run(d, judge_of(config), name, order, store.bits(name, case, n))


def entry_unique_index(d, store, config, control):
    """"unique.algo" = 1 with first_index and inverse: the argsort"""
    def run(dd, judge, name, order, bits, inp, perm):
        exp = store.expected("unique", bits, order, lambda: unique_oracle(bits, name, order))
        run_unique(dd, judge, name, order, bits, inp, exp, True)

    if control is not None:
        control.setParam("unique.algo", 1)
    pair_controls(control, run)
    every_case(d, store, config, run, unique__algo=1)


def entry_reduce_by_key(d, store, config, control):
    """sums of float64 values that are the positions: whole numbers below 2^53 in any partial sum, so exact in any association"""
    def run(dd, judge, name, order, bits, inp, perm):
        n = bits.size
        vals = positions(n, np.float64).view(np.uint64)
        exp = store.expected("reduce_by_key", bits, order, lambda: by_key_oracle(bits, name, order, vals, "f64", SUM))
        vin = Framed(dd, payload=vals, seed=9)
        try:
            run_reduce_by_key(dd, judge, name, order, bits, inp, vals, vin, exp)
        finally:
            vin.release()

    pair_controls(control, run)
    every_case(d, store, config, run)


ENTRIES = [
    ("sort_keys", entry_sort_keys),
    ("sort_pairs", entry_sort_pairs),
    ("argsort", entry_argsort),
    ("topk-full_argsort", entry_topk(False)),
    ("topk-selection", entry_topk(True)),
    ("topk_rows-loop", entry_topk_rows),
    ("sort_rows-flat", entry_sort_rows),
    ("sort_segments-flat", entry_sort_segments),
    ("sort_segments-plan", entry_sort_segments_plan),
    ("unique-keys_path", entry_unique_keys),
    ("unique-index_path", entry_unique_index),
    ("reduce_by_key", entry_reduce_by_key),
]


@pytest.mark.parametrize("config", tf.CONFIG_NAMES)
@pytest.mark.parametrize("entry", [e[1] for e in ENTRIES], ids=[e[0] for e in ENTRIES])
def test_entry_point_under_configuration(dev, store, entry, config):
    with control_handle(config) as control:
        entry(dev, store, config, control)
    # (restored: the next test starts from the default)
    assert dev.getParam("sort.algo") == -1 and dev.getParam("sort.digit_bits") == 8 and dev.getParam("sort.rank") == dev.getParam("sort.lds_ordered")
    assert dev.getParam("debug.resident_wgs") >= 256
    DeviceUtils.waitForCompletion(dev)   # adlhip_sync: no device-side fault


# ---------------------------------------------------------------------------------------------
# knobs changed after the scratch was sized: nothing to refuse
# ---------------------------------------------------------------------------------------------
def every_query(d, n):
    lib = _lib.load()
    out = {}
    for name in ("f32", "f64"):
        kt = BY_NAME[name][1]
        out[name, "sort_keys"] = typed_query(d, kt, 0, 0, n)[2]
        out[name, "sort_pairs"] = typed_query(d, kt, 1, 8, n)[2]
        out[name, "argsort"] = typed_query(d, kt, 2, 0, n)[2]
        for k in tf.topk_ks(n):
            out[name, "topk", k] = query(lib.adlhip_topk_scratch_bytes, d, kt, n, k)
            out[name, "topk_rows", k] = query(lib.adlhip_topk_rows_scratch_bytes, d, kt, 3, n, k)
        out[name, "unique keys path"] = query(lib.adlhip_unique_scratch_bytes, d, kt, n, 0)
        out[name, "unique index path"] = query(lib.adlhip_unique_scratch_bytes, d, kt, n, 1)
        out[name, "reduce_by_key"] = query(lib.adlhip_reduce_by_key_scratch_bytes, d, kt, F64, n)
        out[name, "sort_rows"] = query(lib.adlhip_sort_rows_scratch_bytes, d, kt, 37, n // 37)     # ("sort.rows_algo" = 0 is in force)
        out[name, "sort_segments"] = query(lib.adlhip_sort_segments_scratch_bytes, d, kt, n, 301, 0)   # (no bound: the flat path)
        out[name, "sort_segments plan"] = query(lib.adlhip_sort_segments_scratch_bytes, d, kt, n, tf.PLAN_SEGMENTS, 4096)
    return out


def test_no_configuration_asks_for_more_scratch_than_the_default(dev):
    """Why no entry point has a test of a call refused for knobs changed after its scratch was sized (the module's docstring): such a
    test needs a configuration whose query is strictly larger than the default's, and there is none -- not among the five
    configurations, not with any "sort.tile".  Host only: nothing is enqueued."""
    sizes = sorted(set(tf.PAIR_RUNGS + tf.KEY_RUNGS[4] + tf.KEY_RUNGS[8] + [1000, 16384, 16385]))
    others = [(name, knobs) for name, knobs in tf.CONFIGS[1:]]
    tile = 0
    while True:   # every "sort.tile" the library knows
        try:
            dev.setParam("sort.tile", tile)
        except Exception:
            break
        finally:
            dev.setParam("sort.tile", -1)
        others.append(("tile %d" % tile, [("sort.tile", tile)]))
        tile += 1
    assert tile == 4
    dev.setParam("sort.rows_algo", ROWS_FLAT)   # (the row kernel asks for nothing)
    try:
        for n in sizes:
            base = every_query(dev, n)
            assert min(base.values()) > 0
            for name, knobs in others:
                try:
                    for knob, value in knobs:
                        dev.setParam(knob, value)
                    got = every_query(dev, n)
                finally:
                    dev.setParam("sort.tile", -1)
                    restore(dev)
                    dev.setParam("sort.rows_algo", ROWS_FLAT)
                more = {k: (base[k], v) for k, v in got.items() if v > base[k]}
                assert not more, "n = %d, %s asks for more than the default: %s -- a refusal that can now be tested" % (n, name, more)
    finally:
        restore(dev)
    assert dev.getParam("debug.idle_dirty") == 0
