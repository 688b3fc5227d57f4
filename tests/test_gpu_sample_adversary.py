"""The large sorts on keys built against their own samples (tests/sample_adversary.py has the three samples S, P, B, their position
twins, the key recipes and the case table with every row's derivation).

The suite's other net-driving inputs leave the samples ALMOST right -- one unseen key, two outliers, at positions no sample reads
by chance.  Here what the samples hold says nothing true about the other 97 % of the array: `miss` raised by nearly every workgroup, an
overflow in the first tiles of pass 1, a dictionary of one value probed n times, a net entered from "gave up at the first
instruction" with a wrong `top` and `prefix` in the sample words -- and a handle-owned word left dirty by any of it would change the
NEXT sort, so a friendly sort follows every case on the same handle without a sync in between.

Controls come first: they plant keys AT the twins' positions and one element off and expect the device to tell the two apart.
Without them every case silently degrades into a random-outlier test.
  S  The control as first planned -- ONE key K at all of positions_S, then moved one element on, "expect no net run" -- cannot hold
     in its second half: 2048 copies of one key meet in one segment, whose slab at this n holds 1216 keys for a mean of 768 (adlhip.hip
     msd2_stride_b), so pass 2 overflows and the net runs wherever K sits.  The control therefore plants one key PER WAVE of S (16
     keys in 16 different segments, 128 copies each: the same 16 x 127 repeats on position, +128 keys in a segment off position); K
     alone is run on position as well.
  P  five values and 200 values that occur once, at a P position: the dictionary is complete and the net sorts by counting; one
     element off it misses.
  B  300 values and ~3000 that occur once, at a B position (u32 keys): counting through the big dictionary; one element off, LSD.

Forms, knobs and launch labels are rows of tests/test_gpu_call_sequences.py STATES.  Every handle is fresh (the walk's excepted).
Every call: bit-exact against the suite's numpy oracle, the pristine input copy unchanged, guard regions around the data, the partner
arrays and a work buffer of exactly the queried size, adlhip_fault_check clean, the net's counters as derived, "debug.idle_dirty" 0.

That the controls bite was checked once by hand: with 0x85EBCA6B changed to 0x85EBCA6D in the twin (S and B share that scramble) all
three S controls and both B controls fail, each naming its control ("S control (cursor-friendly), a key per wave at positions_S: (net
runs, counting) = (0, 0), derived from the code: (1, 0)"), the P controls pass, and tests/test_sample_adversary.py fails on the size
of the union.  Wall time of this file on an MI355X: 8 s.

Not covered, on purpose:
  - the mid-size sort: mid_prep_kernel counts EVERY key (four byte histograms of the whole input); there is no sample to lie to it.
  - typed 8-byte keys: their second pair sort runs on an array the first one permuted, so what its samples read is not under the
    test's control.  The typed case runs 4-byte keys only.
"""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP back-end is loaded, as in tests/test_gpu_typed_sort.py)

import oracle
import sample_adversary as sa
import test_gpu_call_sequences as seq
from oclradixsort_amd import DeviceUtils, _lib
from oclradixsort_amd._lib import check
from test_gpu_call_sequences import KV32, SOA32, STATE_BY_NAME, U32, U64
from typed_shapes import ASC, DESC, NAN_PATTERN, encoded_dwords, expected_perm

pytestmark = pytest.mark.gpu

SEED = 20
GUARD = 4096                      # bytes before and behind every buffer (a multiple of the 256-byte alignment)
GUARD_BYTE = 0xC3
NET_LSD, NET_COUNTING, NET_NONE = (1, 0), (1, 1), (0, 0)
KIND_NAME = {U32: "u32", U64: "u64", SOA32: "u32"}

# the forms: rows of STATES (call, kind, n, sort bits, knobs, work level, labels)
FORMS = {
    "cursor": "cursor-friendly",                 # u32, "sort.msd2" 4
    "hybrid": "hybrid-friendly",                 # u32, "sort.msd2" 5
    "stable-u32-24-bits": "stable-u32-24-bits",  # "sort.msd2" 2
    "stable-u64": "stable-u64-binfinish-0",      # whole u64 keys, "sort.msd2" 3 (the stable form, with a dictionary)
    "pairs": "pairs-friendly",                   # kv32, "sort.msd2" 2
    "soa32": "soa32-large",
}
LEVEL2 = "level-2-work-lean"                     # u32, 6 Mi + 3, work level 2


def form_state(form):
    return STATE_BY_NAME[FORMS.get(form, form)]


def kind_of(state):
    """the element kind sample_adversary.build makes for the state (the SoA sort takes u32 keys; its values are the indices)"""
    return "kv32" if state.kind == KV32 else KIND_NAME[state.kind]


def cases_of(state):
    return [c for c in sa.CASES if c.applies(kind_of(state), state.bits)]


# ---------------------------------------------------------------------------------------------
# host side: inputs and references, computed once
# ---------------------------------------------------------------------------------------------
def arrays_of(state, elems):
    """[(name, initial, expected)] of the state's call on `elems` (sa.build's array of the state's kind)"""
    n, bits = state.n, state.bits
    if state.kind == SOA32:
        vals = np.arange(n, dtype=np.uint32)
        order = seq.stable_order(elems, bits)
        return [("keys", elems, elems[order]), ("vals", vals, vals[order])]
    if state.kind == KV32:
        return [("data", elems, oracle.sort_kv32(elems))]
    if state.kind == U64:
        return [("data", elems, oracle.sort_u64(elems) if bits == 64 else elems[seq.stable_order(elems, bits)])]
    return [("data", elems, oracle.sort_u32(elems) if bits == 32 else elems[seq.stable_order(elems, bits)])]


def friendly_arrays(state):
    kind = kind_of(state)
    return arrays_of(state, sa.build(kind, state.n, {}, ("uniform",), SEED + 1))


class Inputs:
    """arrays of (form, case) and of the form's friendly sort; dropped with the form (a case's arrays are up to 50 MB)"""

    def __init__(self, form):
        self.state = form_state(form)
        self._made = {}

    def get(self, case):
        if case not in self._made:
            if case == "friendly":
                self._made[case] = friendly_arrays(self.state)
            else:
                kind = kind_of(self.state)
                self._made[case] = arrays_of(self.state, sa.CASE_BY_NAME[case].build(kind, self.state.n, SEED))
        return self._made[case]


# ---------------------------------------------------------------------------------------------
# device side: a fresh handle, guarded buffers, a work buffer of exactly the queried size
# ---------------------------------------------------------------------------------------------
class GBuf:
    """nbytes on the device between two guards"""

    def __init__(self, dev, nbytes):
        self.dev, self.nbytes, self.total = dev, int(nbytes), int(nbytes) + 2 * GUARD
        self.base = seq.dmalloc(dev, self.total)
        check(_lib.load().adlhip_memset(dev._h, ctypes.c_void_p(self.base), GUARD_BYTE, self.total), "memset")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.base + GUARD)

    def write(self, host):
        b = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        assert b.size == self.nbytes
        check(_lib.load().adlhip_memcpy_h2d(self.dev._h, self.ptr, b.ctypes.data_as(ctypes.c_void_p), b.size), "h2d")

    def copy_from(self, other):
        check(_lib.load().adlhip_memcpy_d2d(self.dev._h, self.ptr, other.ptr, self.nbytes), "d2d")

    def read_all(self):
        """guards and payload; valid after the next sync"""
        out = np.empty(self.total, np.uint8)
        check(_lib.load().adlhip_memcpy_d2h(self.dev._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.base), self.total), "d2h")
        return out

    def read_guards(self):
        out = np.empty(2 * GUARD, np.uint8)
        lib = _lib.load()
        check(lib.adlhip_memcpy_d2h(self.dev._h, out[:GUARD].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.base), GUARD), "d2h")
        check(lib.adlhip_memcpy_d2h(self.dev._h, out[GUARD:].ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.base + GUARD + self.nbytes), GUARD),
              "d2h")
        return out

    def free(self):
        check(_lib.load().adlhip_free(self.dev._h, ctypes.c_void_p(self.base), self.total), "adlhip_free")


def guards_intact(raw, nbytes, what):
    g = np.concatenate([raw[:GUARD], raw[-GUARD:]]) if raw.size != 2 * GUARD else raw
    bad = np.flatnonzero(g != GUARD_BYTE)
    assert bad.size == 0, "%s: %d guard byte(s) written, first %d bytes %s the buffer of %d bytes" % (
        what, bad.size, GUARD - bad[0] if bad[0] < GUARD else bad[0] - GUARD, "before" if bad[0] < GUARD else "behind", nbytes)


class Rig:
    """One fresh handle set up for one form: the state's knobs, `slots` guarded data buffers, guarded partner arrays and a guarded
    work buffer of exactly the size adlhip_radix_sort_scratch_bytes_for states for (kind, n, sort bits, level)."""

    def __init__(self, state, slots, profiled=False):
        self.state, self.lib = state, _lib.load()
        self.dev = DeviceUtils.allocate()
        self.bufs, self.profiled = [], profiled
        try:
            seq.assert_idle(self.dev, "fresh handle")
            seq.set_knobs(self.dev, state.knobs)
            tb, wb = ctypes.c_size_t(), ctypes.c_size_t()
            check(self.lib.adlhip_radix_sort_scratch_bytes_for(self.dev._h, state.kind, state.n, state.bits, state.level, ctypes.byref(tb), ctypes.byref(wb)),
                  "scratch_bytes_for")
            self.work_bytes = wb.value
            esz = seq.ESZ[state.kind]
            self.names = ["keys", "vals"] if state.kind == SOA32 else ["data"]
            self.slots = [{nm: self._buf(state.n * esz) for nm in self.names} for _ in range(slots)]
            self.tmp = [self._buf(state.n * esz) for _ in self.names]
            self.work = self._buf(self.work_bytes)
            self.pristine = {}
            if profiled:
                self.dev.toggleProfiling(True)
        except BaseException:
            self.close()
            raise

    def _buf(self, nbytes):
        b = GBuf(self.dev, nbytes)
        self.bufs.append(b)
        return b

    def close(self):
        self.lib.adlhip_sync(self.dev._h)
        for b in self.bufs:
            b.free()
        if self.profiled:
            self.dev.toggleProfiling(False)
        DeviceUtils.deallocate(self.dev)

    def upload(self, key, arrays):
        """the input's pristine device copy (restore() copies from it; it must come back unchanged)"""
        if key not in self.pristine:
            self.pristine[key] = {}
            for nm, init, _ in arrays:
                b = self._buf(init.nbytes)
                b.write(init)
                self.pristine[key][nm] = b

    def restore(self, key, slot):
        for nm in self.names:
            self.slots[slot][nm].copy_from(self.pristine[key][nm])

    def enqueue(self, slot):
        s, h, d = self.state, self.dev._h, self.slots[slot]
        if s.kind == SOA32:
            return self.lib.adlhip_radix_sort_soa32(h, d["keys"].ptr, d["vals"].ptr, self.tmp[0].ptr, self.tmp[1].ptr, self.work.ptr, self.work_bytes, s.n, s.bits)
        fn = {U32: self.lib.adlhip_radix_sort_u32, KV32: self.lib.adlhip_radix_sort_kv32, U64: self.lib.adlhip_radix_sort_u64}[s.kind]
        return fn(h, d["data"].ptr, self.tmp[0].ptr, self.work.ptr, self.work_bytes, s.n, s.bits)

    def drain(self, what):
        seq.sync(self.dev)
        assert self.lib.adlhip_fault_check(self.dev._h) == 0, "%s: adlhip_fault_check reported: %s" % (what, seq._lib_err())

    def verify(self, jobs, what):
        """jobs: [(slot, pristine key, arrays, rc)].  Outputs bit-exact, pristine copies unchanged, every guard intact."""
        got = [(j, {nm: self.slots[j[0]][nm].read_all() for nm in self.names}) for j in jobs]
        keys = sorted({j[1] for j in jobs})
        kept = {k: {nm: b.read_all() for nm, b in self.pristine[k].items()} for k in keys}
        side = [(b, b.read_guards()) for b in self.tmp + [self.work]]
        seq.sync(self.dev)
        for (slot, key, arrays, rc), raws in got:
            assert rc == 0, "%s, %s: the call failed: %s" % (what, key, seq._lib_err())
            for nm, _, want in arrays:
                raw = raws[nm]
                guards_intact(raw, raw.size - 2 * GUARD, "%s, %s, array '%s'" % (what, key, nm))
                g = raw[GUARD:-GUARD].view(want.dtype)
                if not np.array_equal(g, want):
                    bad = np.flatnonzero(g != want)
                    raise AssertionError("%s, %s: array '%s' differs from the host reference in %d elements, first at %d: got %#x, expected %#x" % (
                        what, key, nm, bad.size, bad[0], int(g[bad[0]]), int(want[bad[0]])))
        for key in keys:
            arrays = next(j[2] for j in jobs if j[1] == key)
            for nm, init, _ in arrays:
                raw = kept[key][nm]
                guards_intact(raw, raw.size - 2 * GUARD, "%s, pristine copy of %s '%s'" % (what, key, nm))
                assert np.array_equal(raw[GUARD:-GUARD].view(init.dtype), init), "%s: the pristine input copy of %s '%s' changed" % (what, key, nm)
        for b, raw in side:
            guards_intact(raw, b.nbytes, "%s, %s" % (what, "work buffer of exactly the queried %d bytes" % b.nbytes if b is self.work else "partner array"))


def run_alone(rig, key, arrays, claim, what, labels=None):
    """The input alone on the rig's handle, synced: the net's counters move as claimed (and the claimed kernels are launched)."""
    dev = rig.dev
    rig.upload(key, arrays)
    rig.restore(key, 0)
    rig.drain(what)
    if rig.profiled:
        dev.profile(reset=True)
    before = seq.net_stats(dev)
    rc = rig.enqueue(0)
    rig.drain(what)
    launched = set(dev.profile(reset=True)) if rig.profiled else set()
    after = seq.net_stats(dev)
    net = (after[0] - before[0], after[1] - before[1])
    print("%-70s (net runs, counting) = %s, claimed %s" % (what, net, claim))
    assert rc == 0, "%s: the call failed: %s" % (what, seq._lib_err())
    assert net == claim, "%s: (net runs, counting) = %s, derived from the code: %s" % (what, net, claim)
    if labels is not None:
        assert labels <= launched, "%s: claimed kernels not launched: %s (launched: %s)" % (what, sorted(labels - launched), sorted(launched))
    rig.verify([(0, key, arrays, rc)], what)
    seq.assert_idle(dev, what)


def run_followed_by_friendly(rig, key, arrays, friendly, claim, what):
    """The input and, WITHOUT a sync in between, a friendly uniform sort on the same handle: both bit-exact, the friendly one adds no
    net run, nothing dirty."""
    dev = rig.dev
    rig.upload(key, arrays)
    rig.upload("friendly", friendly)
    rig.restore(key, 0)
    rig.restore("friendly", 1)
    rig.drain(what)
    before = seq.net_stats(dev)
    rc0 = rig.enqueue(0)
    rc1 = rig.enqueue(1)
    rig.drain(what)
    after = seq.net_stats(dev)
    net = (after[0] - before[0], after[1] - before[1])
    assert net == claim, "%s, then a friendly sort: (net runs, counting) = %s, the case alone %s: the friendly sort met the net" % (what, net, claim)
    rig.verify([(0, key, arrays, rc0), (1, "friendly", friendly, rc1)], what + ", then a friendly sort")
    seq.assert_idle(dev, what + ", then a friendly sort")


def pass_labels(state):
    """the form's sample / pass / offsets kernels (the finish launches under another label when the net has sorted)"""
    return {l for l in state.labels if not l.startswith("segment_sort")}


# ---------------------------------------------------------------------------------------------
# 1. controls: the twins are the device's positions
# ---------------------------------------------------------------------------------------------
def _control(state, name, variants):
    """variants: [(label, elems, claim, labels or None)], each on a fresh handle"""
    for label, elems, claim, labels in variants:
        rig = Rig(state, 1, profiled=labels is not None)
        try:
            run_alone(rig, label, arrays_of(state, elems), claim, "%s control (%s), %s" % (name, state.name, label), labels)
        finally:
            rig.close()


@pytest.mark.parametrize("form", ["cursor", "stable-u64", "pairs"])
def test_S_control(form):
    """On position every wave of S reads 128 copies of its key: 16 x 127 = 2032 repeats >= sample_dup_threshold (98), the passes give up
    and the net runs (P and B show distinct keys: no dictionary, LSD passes).  One element on, the samples read distinct keys and the sort
    is the friendly one: its own kernels, no net.  (One key K at all of S, on position: the net runs too.  Off position it would as
    well -- 2048 equal keys overflow a segment slab -- which is why the control uses a key per wave; module docstring.)"""
    state = form_state(form)
    kind = kind_of(state)
    n, width = state.n, 64 if kind == "u64" else 32
    mk = lambda seen, shift=0: sa.build(kind, n, {"S": seen}, ("uniform",), SEED, shift=shift)
    on, off = mk(("by_wave",)), mk(("by_wave",), 1)
    s_on, s_off = sa.sees(sa.keys_of(kind, on), n, state.bits), sa.sees(sa.keys_of(kind, off), n, state.bits)
    assert s_on.repeats == 2032 >= s_on.threshold == 98 and s_off.repeats < 4, (s_on, s_off)
    _control(state, "S", [
        ("a key per wave at positions_S", on, NET_LSD, pass_labels(state)),
        ("a key per wave at positions_S + 1", off, NET_NONE, state.labels),
        ("one key at positions_S", mk(("one", sa.K_ONE[width])), NET_LSD, None),
    ])


def _with_rare(kind, n, base_values, which, count, off, seed):
    """base_values everywhere and ~count values that occur once, at a position of `which` (off: at its free neighbour)"""
    width = 64 if kind == "u64" else 32
    on_at, off_at = sa.rare_sites(which, n, count)
    table = sa.value_table(base_values + on_at.size, width, seed)
    return sa.build(kind, n, {}, ("values", base_values), seed, extra=[(off_at if off else on_at, table[base_values:])]), on_at.size


@pytest.mark.parametrize("form", ["cursor", "stable-u64", "pairs"])
def test_P_control(form):
    """Five values repeat ~1968 times in S: the passes give up, and >= kDictMinRepeats the net builds its dictionary from P.  The 200
    rare values sit at P positions, so the dictionary holds all 205 and the net sorts by counting (pairs: one stable pass on the
    rank).  One element off no sample reads a rare value: the dictionary holds five, the rare keys raise `miss` (u32 keys: the big
    dictionary of what B shows, five values, misses too) and the LSD passes sort."""
    state = form_state(form)
    kind = kind_of(state)
    n = state.n
    on, rare = _with_rare(kind, n, 5, "P", 200, False, SEED)
    off, _ = _with_rare(kind, n, 5, "P", 200, True, SEED)
    s_on, s_off = sa.sees(sa.keys_of(kind, on), n), sa.sees(sa.keys_of(kind, off), n)
    assert s_on.distinct_P == 5 + rare <= sa.DICT_MAX and s_on.repeats >= sa.DICT_MIN_REPEATS, s_on
    assert s_off.distinct_P == 5 and s_off.distinct_B in (None, 5) and s_off.repeats >= sa.DICT_MIN_REPEATS, s_off
    assert np.unique(sa.keys_of(kind, off)).size == 5 + rare
    _control(state, "P", [
        ("rare values at positions_P", on, NET_COUNTING, None),
        ("rare values one element off positions_P", off, NET_LSD, None),
    ])


@pytest.mark.parametrize("form", ["cursor", "hybrid"])
def test_B_control(form):
    """300 values repeat ~380 times in S: the passes give up; P shows more than 256 values, so the small dictionary is not built; B
    shows the 300 and every rare value (at most 4096 in all): the big dictionary is complete, counting.  One element off B shows 300
    values, the rare keys raise `miss`, LSD passes."""
    state = form_state(form)
    n = state.n
    on, rare = _with_rare("u32", n, 300, "B", 3000, False, SEED)
    off, _ = _with_rare("u32", n, 300, "B", 3000, True, SEED)
    s_on, s_off = sa.sees(on, n), sa.sees(off, n)
    assert s_on.distinct_B == 300 + rare <= sa.BIG_MAX and s_on.distinct_P > sa.DICT_MAX and s_on.repeats >= s_on.threshold, s_on
    assert s_off.distinct_B == 300 and s_off.distinct_P > sa.DICT_MAX and s_off.repeats >= s_off.threshold, s_off
    _control(state, "B", [
        ("rare values at positions_B", on, NET_COUNTING, None),
        ("rare values one element off positions_B", off, NET_LSD, None),
    ])


# ---------------------------------------------------------------------------------------------
# 2. the cases, form by form
# ---------------------------------------------------------------------------------------------
_INPUTS = {}


def inputs_of(form):
    """the form's inputs and references; the tests below run form by form, and the arrays go when the next form begins"""
    if form not in _INPUTS:
        _INPUTS.clear()
        _INPUTS[form] = Inputs(form)
    return _INPUTS[form]


WALK = "all-back-to-back"
# form-major: a form's cases, then its walk.  A case runs on a form only where its premise applies (Case.applies).
CASE_RUNS = [(form, c) for form in FORMS for c in [c.name for c in cases_of(form_state(form))] + [WALK]]


def _case_alone_then_before_a_friendly_sort(state, name, arrays, friendly):
    """Calibration on a fresh handle -- the case alone, synced: the net moves as its row derives (sample_adversary.CASES `why`: the LSD
    passes in every row), the form's kernels are launched -- then the case followed by a friendly sort without a sync."""
    rig = Rig(state, 2, profiled=True)
    try:
        what = "%s on %s" % (name, state.name)
        run_alone(rig, name, arrays, NET_LSD, what, pass_labels(state))
        rig.dev.toggleProfiling(False)
        rig.profiled = False
        run_followed_by_friendly(rig, name, arrays, friendly, NET_LSD, what)
    finally:
        rig.close()


def _cases_back_to_back_on_one_handle(inputs):
    """The form's cases and two friendly sorts in a seeded order, queued on one handle without a sync: the question of
    tests/test_gpu_call_sequences.py, asked of these inputs."""
    state = inputs.state
    names = [c.name for c in cases_of(state)]
    order = names + ["friendly", "friendly"]
    order = [order[i] for i in np.random.default_rng(SEED).permutation(len(order))]
    rig = Rig(state, len(order))
    try:
        for nm in set(order):
            rig.upload(nm, inputs.get(nm))
        for i, nm in enumerate(order):
            rig.restore(nm, i)
        what = "back to back on %s [%s]" % (state.name, " -> ".join(order))
        rig.drain(what)
        before = seq.net_stats(rig.dev)
        rcs = [rig.enqueue(i) for i in range(len(order))]
        rig.drain(what)
        after = seq.net_stats(rig.dev)
        assert (after[0] - before[0], after[1] - before[1]) == (len(names), 0), (what, before, after)
        rig.verify([(i, nm, inputs.get(nm), rcs[i]) for i, nm in enumerate(order)], what)
        seq.assert_idle(rig.dev, what)
    finally:
        rig.close()


@pytest.mark.parametrize("form,case", CASE_RUNS, ids=["%s-%s" % fc for fc in CASE_RUNS])
def test_case(form, case):
    inputs = inputs_of(form)
    if case == WALK:
        _cases_back_to_back_on_one_handle(inputs)
    else:
        _case_alone_then_before_a_friendly_sort(inputs.state, case, inputs.get(case), inputs.get("friendly"))


def test_case_on_the_lean_work_level():
    """6 Mi + 3 u32 keys on work level 2 (slabs with 12 % head-room; sample_dup_threshold = 50): case 2, the passes give up and both
    dictionaries, of one value each, miss."""
    state = STATE_BY_NAME[LEVEL2]
    case = sa.CASE_BY_NAME["2-one-key-seen-uniform-rest"]
    elems = case.build("u32", state.n, SEED)
    s = sa.check_premise(case, elems, state.n, 32)
    assert s.threshold == 50, s
    rig = Rig(state, 2, profiled=True)
    try:
        what = "%s on %s" % (case.name, state.name)
        arrays = arrays_of(state, elems)
        run_alone(rig, case.name, arrays, NET_LSD, what, pass_labels(state))
        rig.dev.toggleProfiling(False)
        rig.profiled = False
        run_followed_by_friendly(rig, case.name, arrays, friendly_arrays(state), NET_LSD, what)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------
# 3. one typed case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ASC, DESC], ids=["asc", "desc"])
def test_argsort_f32_with_nan_at_every_sampled_position(order):
    """adlhip_argsort_typed sorts {encoded key, index} pairs with the stable pair sort, whose samples read the pair at the sampled
    INDEX: +NaN at S, P and B, standard normals elsewhere.  Every sample reads one value (the largest ascending, the smallest
    descending), the passes give up, the pair dictionary of one value misses, the LSD passes sort: (net runs, counting) = (1, 0).
    4-byte keys only: the second pair sort of 8-byte keys runs on a permuted array, its samples are not the test's to place."""
    n = seq.N_LARGE
    x = np.random.default_rng(SEED).standard_normal(n).astype(np.float32)
    bits = x.view(np.uint32).copy()
    bits[sa.union_positions(n)] = NAN_PATTERN[4]
    enc, _ = encoded_dwords(bits, "f32")
    s = sa.sees(enc if order == ASC else ~enc, n)
    assert s.repeats == 2032 and s.distinct_P == 1 and s.distinct_B == 1, s
    want = expected_perm(bits, "f32", order).astype(np.uint32)
    lib = _lib.load()
    dev = DeviceUtils.allocate()
    bufs = []
    try:
        a, b, wb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        check(lib.adlhip_sort_typed_scratch_bytes(dev._h, 2, 2, 0, n, ctypes.byref(a), ctypes.byref(b), ctypes.byref(wb)), "typed scratch")
        kin, kout, idx, work = (GBuf(dev, nb) for nb in (4 * n, 4 * n, 4 * n, wb.value))
        bufs = [kin, kout, idx, work]
        kin.write(bits)
        seq.sync(dev)
        before = seq.net_stats(dev)
        rc = lib.adlhip_argsort_typed(dev._h, 2, order, kin.ptr, kout.ptr, idx.ptr, work.ptr, wb.value, n)
        assert rc == 0, seq._lib_err()
        seq.sync(dev)
        assert lib.adlhip_fault_check(dev._h) == 0, seq._lib_err()
        after = seq.net_stats(dev)
        raws = [x_.read_all() for x_ in (kin, kout, idx)] + [work.read_guards()]
        seq.sync(dev)
        for raw, buf, nm in zip(raws, bufs, ("keys in", "keys out", "index out", "work")):
            guards_intact(raw, buf.nbytes, "typed argsort, " + nm)
        assert np.array_equal(raws[0][GUARD:-GUARD].view(np.uint32), bits), "argsort changed d_keys_in"
        got = raws[2][GUARD:-GUARD].view(np.uint32)
        assert np.array_equal(got, want), "index differs from the stable order in %d places" % np.count_nonzero(got != want)
        assert np.array_equal(raws[1][GUARD:-GUARD].view(np.uint32), bits[want])
        assert (after[0] - before[0], after[1] - before[1]) == NET_LSD, (before, after)
        seq.assert_idle(dev, "typed argsort")
    finally:
        lib.adlhip_sync(dev._h)
        for buf in bufs:
            buf.free()
        DeviceUtils.deallocate(dev)
