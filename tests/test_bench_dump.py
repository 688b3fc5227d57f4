"""bench.py --dump-outputs: the files it writes for comparing two builds output for output (host side only)."""
import numpy as np

import bench


def test_dump_outputs_are_exact_float64_and_bounded(tmp_path):
    n = (1 << 22) + 5
    keys = np.sort(np.random.default_rng(1).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32))
    keys[-1] = 0xffffffff
    bench.dump_outputs(str(tmp_path), "sorted_keys", keys)
    sample = np.load(tmp_path / "sorted_keys_sample.npy")
    idx = np.load(tmp_path / "sorted_keys_sample_index.npy")
    sums = np.load(tmp_path / "sorted_keys_block_sums.npy")
    assert sample.dtype == idx.dtype == sums.dtype == np.float64
    assert sample.size == idx.size == bench.DUMP_SAMPLE
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(sample, keys[idx.astype(np.int64)].astype(np.float64))
    want = [int(keys[i:i + bench.DUMP_BLOCK].astype(np.uint64).sum()) for i in range(0, n, bench.DUMP_BLOCK)]
    assert [int(v) for v in sums] == want
    # the sample positions are fixed: a second dump of other keys of the same size samples the same places
    other = tmp_path / "again"
    bench.dump_outputs(str(other), "sorted_keys", keys[::-1].copy())
    assert np.array_equal(np.load(other / "sorted_keys_sample_index.npy"), idx)
    # at the benchmark's size (64 Mi keys) everything stays far below 64 MB
    total = 8 * (2 * bench.DUMP_SAMPLE + (bench.N_KEYS + bench.DUMP_BLOCK - 1) // bench.DUMP_BLOCK)
    assert total <= 64 * 10 ** 6


def test_dump_outputs_of_a_small_or_empty_slice(tmp_path):
    keys = np.arange(10, dtype=np.uint32)
    bench.dump_outputs(str(tmp_path), "sorted_keys_rank1", keys, share=4)
    assert np.array_equal(np.load(tmp_path / "sorted_keys_rank1_sample.npy"), keys.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "sorted_keys_rank1_block_sums.npy"), [45.0])
    bench.dump_outputs(str(tmp_path), "empty", np.zeros(0, dtype=np.uint32))
    assert np.load(tmp_path / "empty_sample.npy").size == 0
    assert np.load(tmp_path / "empty_block_sums.npy").size == 0
