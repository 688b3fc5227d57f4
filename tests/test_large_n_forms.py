"""The closed forms of tests/large_n.py against numpy's own results at small sizes, and the verifier against planted errors (no GPU).

tests/test_gpu_large_n.py trusts these forms at sizes where no host reference is affordable; here every form is evaluated on CPU
tensors at 10^4 .. 10^5 elements (tails included) and compared with np.sort, stable argsort, np.unique, np.cumsum,
np.maximum.accumulate, np.bincount, np.histogram, np.searchsorted, intersect1d / union1d / setdiff1d / setxor1d and the stable
argsort of a concatenation.  The second half plants one wrong element in a correct result -- a flipped bit, two swapped indices among
equal keys, a duplicated index, a count off by one -- and demands that the verifier raises and names that element.
"""
import numpy as np
import pytest
import torch

import large_n as L
import typed_shapes

CPU = torch.device("cpu")
SIZES = [100003, 65536, 10007]


@pytest.fixture(autouse=True)
def _small_chunks():
    """chunks far smaller than the arrays, so that every chunk boundary of fill() and the checks is walked"""
    old = L.CHUNK
    L.CHUNK = 4099
    yield
    L.CHUNK = old


def ev(form, n):
    return form(L.arange(0, n, CPU)).numpy()


def tensor_of(form, n, dtype):
    return L.fill(torch.empty(n, dtype=dtype), form)


def bits_np(t, ktype):
    """a filled tensor as numpy bit patterns of the type's unsigned twin"""
    return t.numpy().view(np.uint32 if t.dtype == torch.int32 else np.uint64)


def np_stable_order(bits, ktype, order):
    return typed_shapes.expected_perm(bits, ktype, order)


def is_prime(p):
    return p > 1 and all(p % d for d in range(2, int(p ** 0.5) + 1))


def test_prime_and_permutation():
    assert is_prime(L.PRIME_A) and L.PRIME_A < (1 << 31)
    for n in SIZES + [1, 2, 97]:
        p = L.Perm(n)
        v = ev(p, n)
        assert np.array_equal(np.sort(v), np.arange(n))
        assert np.array_equal(ev(p.inv, n), np.argsort(v, kind="stable"))


def test_permutation_inverse_at_the_top_of_the_range():
    """the products of Perm stay below 2^63 at the largest n: spot values against python integers"""
    n = 0xFFF00000
    p = L.Perm(n)
    i = torch.tensor([0, 1, 12345, (1 << 31) - 1, 1 << 31, n - 2, n - 1], dtype=torch.int64)
    want = [(int(x) * p.a + p.b) % n for x in i]
    assert p(i).tolist() == want
    assert p.inv(torch.tensor(want, dtype=torch.int64)).tolist() == i.tolist()


@pytest.mark.parametrize("ktype", list(L.KEY_TYPES))
def test_ordinal_to_bits_is_the_order_typed_shapes_states(ktype):
    """rising ordinals give keys that rise strictly in the order typed_shapes.ordinal_halves states, over sign changes, +-0 and NaNs"""
    if L.key_bytes(ktype) == 4:
        o = torch.cat([torch.arange(0, 5000), torch.arange(L.S32 - 5000, L.S32 + 5000), torch.arange((1 << 32) - 5000, 1 << 32),
                       torch.arange(0x7f800000 - 100 + L.S32, 0x7f800000 + 100 + L.S32)]).sort().values
        bits = L.to_i32(L.ordinal_to_bits(o, ktype)).numpy().view(np.uint32)
    else:
        o = torch.cat([torch.arange(L.MIN64, L.MIN64 + 5000), torch.arange(-5000, 5000), torch.arange((1 << 63) - 5000, (1 << 62) * 2 - 1),
                       torch.arange(0x7ff0000000000000 - 100, 0x7ff0000000000000 + 100)]).sort().values
        bits = L.ordinal_to_bits(o, ktype).numpy().view(np.uint64)
    hi, lo = typed_shapes.ordinal_halves(bits, ktype)
    step_hi, step_lo = np.diff(hi), np.diff(lo)
    assert np.all((step_hi > 0) | ((step_hi == 0) & (step_lo > 0)))
    if ktype[0] == "f":
        f = bits.view(np.float32 if bits.dtype == np.uint32 else np.float64)
        assert np.isnan(f).any() and (bits == (1 << (8 * bits.dtype.itemsize - 1))).any()   # NaNs and -0 occur


@pytest.mark.parametrize("order", [L.ASC, L.DESC])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("ktype", list(L.KEY_TYPES))
def test_sort_form(ktype, shift, order):
    for n in SIZES[:2]:
        f = L.SortForm(n, ktype, order, shift)
        dt = torch.int32 if L.key_bytes(ktype) == 4 else torch.int64
        kin = tensor_of(f.keys_in, n, dt)
        bits = bits_np(kin, ktype)
        perm = np_stable_order(bits, ktype, order)
        L.check_equal(torch.from_numpy(bits[perm].view(np.int32 if dt == torch.int32 else np.int64)), f.keys_out, n, "keys")
        index = torch.from_numpy(perm.astype(np.uint32).view(np.int32))
        if shift == 0:
            L.check_equal(index, f.index_out, n, "index")
        L.check_gather(index, f.keys_in, f.keys_out, n, n, "index")
        L.check_rising(index, f.keys_out, n, "index")
        if L.key_bytes(ktype) == 8:   # both dwords vary
            assert np.unique(bits >> np.uint64(32)).size > n // 64 and np.unique(bits & np.uint64(0xffffffff)).size > n // 64


def test_runs():
    for n in SIZES + [1, 5, 6, 16]:
        r = L.Runs(n)
        key = ev(r.key, n)
        u, first, counts = np.unique(key, return_index=True, return_counts=True)
        assert r.num_runs == u.size and np.array_equal(u, np.arange(u.size))
        R = u.size
        assert np.array_equal(ev(r.offsets, R + 1), np.append(first, n))
        assert np.array_equal(ev(r.counts, R), counts)
        assert set(counts[:-1]) <= {5, 6}
        pos = np.arange(n, dtype=np.int64)
        assert np.array_equal(ev(r.sum_of_positions, R), np.add.reduceat(pos, first))
        assert np.array_equal(ev(r.min_of_positions, R), np.minimum.reduceat(pos, first))
        assert np.array_equal(ev(r.max_of_positions, R), np.maximum.reduceat(pos, first))
        assert np.array_equal(ev(r.count_so_far, n), pos - first[key] + 1)


def test_scans():
    for n in SIZES:
        x = ev(L.scan_sum_in, n)
        assert np.array_equal(ev(L.scan_sum_out, n), np.cumsum(x))
        assert np.array_equal(ev(L.scan_sum_exclusive_out(1000), n), 1000 + np.cumsum(x) - x)
        assert np.array_equal(ev(L.scan_max_out, n), np.maximum.accumulate(ev(L.scan_max_in, n)))
        assert np.array_equal(ev(L.scan_min_out(n), n), np.minimum.accumulate(ev(L.scan_min_in(n), n)))
        assert ev(L.scan_min_in(n), n).min() >= 0


def test_histograms():
    for n in SIZES:
        for bins in (7, 256, 4096, 50000):
            assert np.array_equal(ev(L.bincount_out(n, bins), bins), np.bincount(ev(L.bincount_in(n, bins), n), minlength=bins))
        for bins in (1, 3, 7, 4096):
            e = ev(L.edges(n, bins), bins + 1)
            assert np.all(np.diff(e) >= 0) and e[0] > 0 and e[-1] < n
            keys = ev(L.Perm(n), n)
            want = np.histogram(keys[keys != e[-1]], bins=e)[0]   # numpy closes the last bin; the half-open contract does not
            assert np.array_equal(ev(L.histogram_range_out(n, bins), bins), want)


def test_compaction():
    for n in SIZES + [1, 2, 3, 4]:
        flags = ev(L.flags_in, n)
        sel = np.flatnonzero(flags)
        rej = np.flatnonzero(flags == 0)
        c = L.flagged_count(n)
        assert c == sel.size
        assert np.array_equal(ev(L.flagged_index_out, c), sel)
        assert np.array_equal(L.rejected_index_out(n)(L.arange(c, n, CPU)).numpy(), rej)


@pytest.mark.parametrize("na,nb", [(60001, 40002), (40002, 60001), (40001, 60000), (50001, 50001), (50000, 50000), (60000, 40001), (7, 0),
                                   (0, 7), (1, 1)])
def test_merge(na, nb):
    a, b = ev(L.merge_in, na), ev(L.merge_in, nb)
    cat = np.concatenate([a, b])
    want = np.argsort(cat, kind="stable")
    m = L.Merge(na, nb)
    assert np.array_equal(ev(m.source, na + nb), want)
    assert np.array_equal(ev(m.keys_out, na + nb), cat[want])


@pytest.mark.parametrize("na,nb", [(60000, 40000), (45000, 40000), (30000, 40000), (30001, 20001), (6, 4), (1, 1)])
def test_set_operations(na, nb):
    a, b = 2 * np.arange(na, dtype=np.int64), 3 * np.arange(nb, dtype=np.int64)
    s = L.SetOps(na, nb)
    for op, fn in (("intersection", np.intersect1d), ("union", np.union1d), ("difference", np.setdiff1d),
                   ("symmetric_difference", np.setxor1d)):
        want = fn(a, b)
        assert s.count(op) == want.size, op
        assert np.array_equal(ev(s.keys_out(op), want.size), want), op
        src = ev(s.source(op), want.size)
        assert np.array_equal(np.concatenate([a, b])[src], want), op
        in_a = np.isin(want, a)
        assert np.all(src[in_a] < na) and np.all(src[~in_a] >= na), op   # an element of both inputs is A's


def test_search():
    for m in SIZES:
        h = ev(L.haystack, m)
        q = np.arange(0, h[-1] + 10, dtype=np.int64)
        qt = torch.from_numpy(q)
        assert np.array_equal(L.search_left(m)(qt).numpy(), np.searchsorted(h, q, side="left"))
        assert np.array_equal(L.search_right(m)(qt).numpy(), np.searchsorted(h, q, side="right"))


@pytest.mark.parametrize("order", [L.ASC, L.DESC])
def test_rows(order):
    rows = 3001
    r = L.Rows32(rows, order)
    k = ev(r.keys_in, rows * 32).reshape(rows, 32)
    o = np.argsort(k if order == L.ASC else -k, axis=1, kind="stable")
    assert np.array_equal(ev(r.keys_out, rows * 32).reshape(rows, 32), np.take_along_axis(k, o, 1))
    assert np.array_equal(ev(r.index_out, rows * 32).reshape(rows, 32), o)
    cols, stride = 4099, 4103
    p = L.RowsPrime(23, cols, order=order, stride=stride)
    full = ev(p.keys_in_strided, 23 * stride).reshape(23, stride)
    assert np.all(full[:, cols:] == 0x7fffffff)
    k = full[:, :cols]
    o = np.argsort(k if order == L.ASC else -k, axis=1, kind="stable")
    assert np.array_equal(ev(p.keys_out, 23 * cols).reshape(23, cols), np.take_along_axis(k, o, 1))
    f = L.arange(0, 23 * cols, CPU)
    assert np.array_equal(p.key_at_index(f, torch.from_numpy(o.reshape(-1))).numpy(), ev(p.keys_out, 23 * cols))


@pytest.mark.parametrize("order", [L.ASC, L.DESC])
@pytest.mark.parametrize("dup", [0, 1])
@pytest.mark.parametrize("long_first", [0, 5003])
def test_segments(long_first, dup, order):
    s = L.Segments(11, long_first=long_first, order=order, dup=dup)
    off = ev(s.offsets, s.S + 1)
    assert off[0] == 0 and off[-1] == s.n and np.all(np.diff(off) >= 0) and (np.diff(off) == 0).any()
    assert np.diff(off).max() == s.max_segment
    seg_of = np.searchsorted(off[1:], np.arange(s.n), side="right")
    assert np.array_equal(ev(s.segment_start, s.n), off[seg_of])
    k = ev(s.keys_in, s.n)
    want = np.empty_like(k)
    for a, b in zip(off[:-1], off[1:]):
        seg = k[a:b]
        want[a:b] = seg[np.argsort(seg if order == L.ASC else -seg, kind="stable")]
    assert np.array_equal(ev(s.keys_out, s.n), want)


# ---------------------------------------------------------------------------------------------------------------------
# the verifier against planted errors
# ---------------------------------------------------------------------------------------------------------------------
N = 100003
SPOTS = [0, 4098, 4099, 54321, N - 1]   # the first element, both sides of a chunk boundary, the middle, the last


def _sorted_case(shift):
    f = L.SortForm(N, "i32", L.ASC, shift)
    kin = tensor_of(f.keys_in, N, torch.int32)
    perm = np_stable_order(bits_np(kin, "i32"), "i32", L.ASC)
    return f, tensor_of(f.keys_out, N, torch.int32), torch.from_numpy(perm.astype(np.uint32).view(np.int32)).clone()


@pytest.mark.parametrize("at", SPOTS)
@pytest.mark.parametrize("bit", [0, 31])
def test_verifier_names_one_flipped_bit(at, bit):
    f, kout, _ = _sorted_case(0)
    L.check_equal(kout, f.keys_out, N, "keys")
    kout[at] ^= (1 << bit) if bit < 31 else -(1 << 31)
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(kout, f.keys_out, N, "keys")
    assert e.value.index == at and e.value.got ^ e.value.want == 1 << bit
    wide = tensor_of(L.SortForm(N, "f64").keys_out, N, torch.int64)
    wide[at] ^= 1 << 40
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(wide, L.SortForm(N, "f64").keys_out, N, "keys")
    assert e.value.index == at


def test_checksum_sees_one_flipped_bit_and_a_swap():
    f, kout, _ = _sorted_case(3)
    want = L.form_checksum(f.keys_out, N, CPU, torch.int32)
    assert L.checksum(kout, N) == want
    kout[777] ^= 4
    assert L.checksum(kout, N) != want
    kout[777] ^= 4
    kin = tensor_of(f.keys_in, N, torch.int32)
    assert L.checksum(kin, N) == L.form_checksum(f.keys_in, N, CPU, torch.int32)
    kin[[5, 6]] = kin[[6, 5]]
    assert L.checksum(kin, N) != L.form_checksum(f.keys_in, N, CPU, torch.int32)


@pytest.mark.parametrize("at", [0, 4096, 54320, N - 3 - 8])
def test_verifier_names_two_swapped_indices_among_equal_keys(at):
    f, _, index = _sorted_case(3)   # keys_out[j] = base + (j >> 3): slots at, at + 1 (at a multiple of 8) hold one key
    assert at % 8 == 0
    L.check_gather(index, f.keys_in, f.keys_out, N, N, "index")
    L.check_rising(index, f.keys_out, N, "index")
    index[[at + 2, at + 3]] = index[[at + 3, at + 2]]
    L.check_gather(index, f.keys_in, f.keys_out, N, N, "index")   # the swap keeps the gather property: only the order can tell
    with pytest.raises(L.Mismatch) as e:
        L.check_rising(index, f.keys_out, N, "index")
    assert e.value.index == at + 3


def test_verifier_names_a_swap_across_a_chunk_boundary():
    f, _, index = _sorted_case(13)   # runs of 8192 slots: the pair (4098, 4099) straddles two chunks inside one run
    index[[4098, 4099]] = index[[4099, 4098]]
    with pytest.raises(L.Mismatch) as e:
        L.check_rising(index, f.keys_out, N, "index")
    assert e.value.index == 4099


@pytest.mark.parametrize("at", [1, 4099, 54321, N - 1])
def test_verifier_names_a_duplicated_index(at):
    f, _, index = _sorted_case(3)
    index[at] = index[at - 1]   # among equal keys (at is no multiple of 8): the gather property holds, the indices do not rise
    assert at % 8 != 0
    L.check_gather(index, f.keys_in, f.keys_out, N, N, "index")
    with pytest.raises(L.Mismatch) as e:
        L.check_rising(index, f.keys_out, N, "index")
    assert e.value.index == at
    g, _, exact = _sorted_case(0)   # distinct keys: a duplicated index points at a wrong key
    exact[at] = exact[at - 1]
    with pytest.raises(L.Mismatch) as e:
        L.check_gather(exact, g.keys_in, g.keys_out, N, N, "index")
    assert e.value.index == at
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(exact, g.index_out, N, "index")
    assert e.value.index == at


def test_verifier_names_an_index_out_of_range():
    f, _, index = _sorted_case(3)
    index[4100] = N   # one past the end
    with pytest.raises(L.Mismatch) as e:
        L.check_gather(index, f.keys_in, f.keys_out, N, N, "index")
    assert e.value.index == 4100


@pytest.mark.parametrize("delta", [1, -1])
def test_verifier_names_a_count_off_by_one(delta):
    r = L.Runs(N)
    word = torch.tensor([r.num_runs], dtype=torch.int32)
    L.check_count(word, r.num_runs, "runs")
    word[0] += delta
    with pytest.raises(L.Mismatch) as e:
        L.check_count(word, r.num_runs, "runs")
    assert e.value.got == r.num_runs + delta and e.value.want == r.num_runs
    counts = tensor_of(r.counts, r.num_runs, torch.int32)
    counts[9000] += delta
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(counts, r.counts, r.num_runs, "counts")
    assert e.value.index == 9000
    hist = tensor_of(L.bincount_out(N, 4096), 4096, torch.int32)
    hist[4095] += delta
    with pytest.raises(L.Mismatch) as e:
        L.check_equal(hist, L.bincount_out(N, 4096), 4096, "bincount")
    assert e.value.index == 4095


def test_rising_everywhere_names_a_repeated_position():
    """select_if and partition: positions rise strictly over the whole selected stretch"""
    index = L.to_i32(L.flagged_index_out(L.arange(0, 30000, CPU))).clone()
    L.check_rising(index, None, 30000, "select", everywhere=True)
    index[8198] = index[8197]
    with pytest.raises(L.Mismatch) as e:
        L.check_rising(index, None, 30000, "select", everywhere=True)
    assert e.value.index == 8198


def test_u32_results_are_read_unsigned():
    t = torch.tensor([-1, -(1 << 31), 5], dtype=torch.int32)
    assert L.from_u32(t).tolist() == [0xffffffff, 0x80000000, 5]
    L.check_equal(t, lambda i: torch.tensor([0xffffffff, 0x80000000, 5])[i], 3, "u32")
    assert L.to_i32(torch.tensor([0xffffffff, 0x80000000, 5, (7 << 32) + 9])).tolist() == [-1, -(1 << 31), 5, 9]


def test_groups():
    for n, m in ((100003, 20011), (65536, 65536), (10007, 1)):
        g = L.Groups(n, m)
        key = ev(g.key, n)
        u, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
        assert np.array_equal(u, np.arange(m))
        assert np.array_equal(ev(g.first_index, m), first)
        assert np.array_equal(ev(g.counts, m), counts)
        assert np.array_equal(key, inverse.reshape(-1))
        assert np.array_equal(ev(g.sum_of_positions, m), np.bincount(key, weights=np.arange(n)).astype(np.int64))
