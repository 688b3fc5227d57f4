"""tests/sample_adversary.py on the CPU: the position twins stay inside their cells and never read an element twice, and every
recipe of the case table and of the controls shows the samples what its row claims (tests/test_gpu_sample_adversary.py then runs them
on the device, where the controls prove that the twins are the device's positions)."""
import numpy as np
import pytest

import sample_adversary as sa

Mi = 1 << 20
N_LARGE = 3 * Mi + 17        # tests/test_gpu_call_sequences.py N_LARGE (that module needs the native library: not imported here)
N_LEVEL2 = 6 * Mi + 3
SEED = 20


def _probe_sizes():
    """the sizes of tests/test_gpu_parity.py test_probe_sample_positions_stay_inside_the_array"""
    rng = np.random.RandomState(5)
    sizes = [16384, 16385, 20543, 730669, 7726351, (1 << 24) - 1, 1 << 26, (1 << 28) + 12345, (1 << 30) + 7]
    return sizes + [int(2 ** rng.uniform(14.1, 30)) for _ in range(300)]


@pytest.mark.parametrize("which", ["S", "P", "B"])
def test_positions_lie_inside_their_cells_and_are_distinct(which):
    floor = {"S": sa.S_SAMPLES, "P": sa.P_SAMPLES, "B": sa.BIG_MIN_N}[which]
    for n in [N_LARGE, N_LEVEL2] + [n for n in _probe_sizes() if n >= floor]:
        at = sa.POSITIONS[which](n)
        lo, hi = sa.cell_bounds(which, n)
        assert at.size == sa.CELLS[which]
        assert np.all(at >= lo) and np.all(at < np.maximum(hi, lo + 1)) and at.max() < n, (which, n)
        assert np.all(np.diff(at) > 0), (which, n)      # ascending and distinct: cell k lies before cell k + 1


def test_the_sets_at_the_large_states_size():
    s, p, b = sa.positions_S(N_LARGE), sa.positions_P(N_LARGE), sa.positions_B(N_LARGE)
    assert (np.unique(s).size, np.unique(p).size, np.unique(b).size) == (2048, 16384, 65536)
    u = sa.union_positions(N_LARGE)
    assert u.size == 83569                               # the sets overlap in a few hundred places; 2.66 % of n
    assert 0 < 2048 + 16384 + 65536 - u.size < 1000
    assert sa.sample_dup_threshold(N_LARGE) == 98
    assert sa.sample_dup_threshold(64 * Mi) == 4 and sa.sample_dup_threshold(N_LEVEL2) == 50


def test_overlaps_go_to_S_then_P_then_B():
    n = N_LARGE
    k = sa.build("u32", n, {"S": ("one", 1), "P": ("one", 2), "B": ("one", 3)}, ("one", 0), SEED)
    s, p, b = sa.positions_S(n), sa.positions_P(n), sa.positions_B(n)
    assert np.all(k[s] == 1)
    assert np.all(k[np.setdiff1d(p, s)] == 2) and np.all(k[np.setdiff1d(b, np.union1d(s, p))] == 3)
    assert np.count_nonzero(k) == sa.union_positions(n).size
    pairs = sa.build("kv32", n, {"S": ("one", 7)}, ("uniform",), SEED)
    assert np.array_equal(pairs >> np.uint64(32), np.arange(n, dtype=np.uint64))        # the value is the element's index
    assert np.array_equal(sa.keys_of("kv32", pairs), sa.build("u32", n, {"S": ("one", 7)}, ("uniform",), SEED))
    u = sa.build("u64", n, {}, ("uniform",), SEED)
    assert np.unique(u).size == n and np.unique(sa.build("u32", n, {}, ("uniform",), SEED)).size == n   # "uniform" = distinct


FORMS = [("u32", 32), ("u32", 24), ("u64", 64), ("kv32", 32)]      # (kind, sort bits) of the forms the GPU file runs


@pytest.mark.parametrize("case", sa.CASES, ids=[c.name for c in sa.CASES])
def test_every_case_shows_the_samples_what_its_row_claims(case):
    ran = 0
    for kind, bits in FORMS:
        if not case.applies(kind, bits):
            continue
        for n in (N_LARGE, N_LEVEL2) if (kind, bits) == ("u32", 32) else (N_LARGE,):
            keys = sa.keys_of(kind, case.build(kind, n, SEED))
            s = sa.check_premise(case, keys, n, bits)
            # the premise of the whole file: what the samples hold says nothing true about the rest
            rest = np.delete(keys, sa.union_positions(n))
            seen_vals = np.unique(keys[sa.union_positions(n)])
            # (case 4: 256 of the rest's 300 values are the sampled ones; elsewhere at most one key in a thousand is a sampled value)
            assert np.count_nonzero(np.isin(rest, seen_vals)) <= (0.9 if case.name.startswith("4-") else 0.001) * rest.size, (case.name, kind, s)
            ran += 1
    assert ran


def test_S_control_premises():
    for kind, bits in (("u32", 32), ("u64", 64), ("kv32", 32)):
        n = N_LARGE
        on = sa.sees(sa.keys_of(kind, sa.build(kind, n, {"S": ("by_wave",)}, ("uniform",), SEED)), n, bits)
        off = sa.sees(sa.keys_of(kind, sa.build(kind, n, {"S": ("by_wave",)}, ("uniform",), SEED, shift=1)), n, bits)
        one = sa.sees(sa.keys_of(kind, sa.build(kind, n, {"S": ("one", sa.K_ONE[32])}, ("uniform",), SEED)), n, bits)
        assert on.repeats == 2032 == one.repeats and on.threshold == 98
        assert off.repeats < 4 and off.top == bits, off          # one element off: (nearly) no sample reads a planted key
        assert on.distinct_P > sa.DICT_MAX and (on.distinct_B is None or on.distinct_B > sa.BIG_MAX)
    w = sa.wave_keys(32)
    assert np.unique(w >> np.uint64(28)).size == 16 and np.unique((w >> np.uint64(20)) & np.uint64(15)).size == 16
    assert np.unique(sa.wave_keys(64) >> np.uint64(60)).size == 16


def test_rare_sites_cover_the_first_and_the_last_cell():
    n = N_LARGE
    u = sa.union_positions(n)
    for which, count, least in (("P", 200, 195), ("B", 3000, 2950)):
        on, off = sa.rare_sites(which, n, count)
        at = sa.POSITIONS[which](n)
        assert least <= on.size <= count and on[0] == at[0] and on[-1] == at[-1], (which, on.size)
        assert np.all(np.isin(on, at)) and not np.any(np.isin(off, u)) and np.all(np.abs(off - on) == 1)
        assert np.unique(on).size == on.size and np.unique(off).size == off.size
