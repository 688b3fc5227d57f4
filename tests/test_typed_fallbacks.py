"""tests/typed_fallbacks.py on the CPU: the configurations and sizes are the ones the suite means to run, the shapes have the properties
their tests rely on, and the label rules accept what each configuration launches and refuse what it must not (the label sets are those
of tests/test_gpu_parity.py, tests/test_gpu_call_sequences.py and tests/test_gpu_typed_shapes.py, spelled out so that no GPU module is
imported here)."""
import re
from pathlib import Path

import numpy as np
import pytest

import typed_fallbacks as tf
import typed_shapes
from typed_fallbacks import Sort

ROOT = Path(__file__).resolve().parent.parent

TYPED64 = {"typed_pack_index_k64", "typed_repack_high", "typed_gather"}
TYPED32 = {"typed_pack_index_k32", "typed_gather"}
SMALL = {"small_sort_e64"}
MID3 = {"mid_prep_e64", "onesweep_e64_8b", "segment_sort_e64"}
MID2 = {"mid_bucket_scatter_u32", "segment_sort_u32"}
LARGE_PAIRS = {"msd2s_prep", "msd2s_pass1_kv32", "msd2s_pass2_kv32", "msd2s_offsets", "segment_sort_wave_e64"}
LARGE_U32 = {"msd2_sample", "msd2_pass1_u32", "msd2_pass2_u32", "msd2_offsets", "segment_sort_wave_u32"}
PASSES8 = {"count_e64_8b", "scan_table", "scatter_e64_8b"}
PASSES8_U32 = {"count_u32_8b", "scan_table", "scatter_u32_8b"}
PASSES4 = {"count_e64_4b", "scan_table", "scatter_e64_4b"}
ONE_SWEEP = {"os_hist_e64", "os_hist_reduce", "os_tables", "onesweep_e64_8b"}
SOA8 = {"count_soa_8b", "scan_table", "scatter_soa_8b"}
ROWS = {"rows_pack", "rows_of_positions", "rows_emit"}
MID_N, TOP_N = tf.PAIR_RUNGS[1], tf.PAIR_RUNGS[2]


def refused(config, labels, sorts, net_delta=(0, 0)):
    with pytest.raises(AssertionError):
        tf.check_labels(config, labels, sorts, net_delta)


def test_the_constants_are_those_of_the_library():
    csrc = ROOT / "oclradixsort_amd" / "csrc"   # the large sort's limits, and kSmallMax with them, are large_plan.hpp's
    src = (csrc / "adlhip.hip").read_text() + (csrc / "large_plan.hpp").read_text()

    def const(name):
        m = re.search(r"constexpr size_t %s = ([^;]+);" % name, src)
        assert m, name
        expr = m.group(1).strip()
        if expr in ("kSmallMax",):
            return const(expr)
        m = re.fullmatch(r"size_t\((\d+)\) << (\d+)", expr)
        return int(m.group(1)) << int(m.group(2)) if m else int(expr)

    assert const("kSmallMax") == tf.SMALL_MAX
    assert const("kMidMinU32") == tf.MID_MIN_U32
    assert const("kMidMaxE64") == const("kMsd2sAutoMin") == tf.MID_MAX_E64
    assert const("kMidMaxU32") == const("kMsd2AutoMin") == tf.MID_MAX_U32


def test_the_rungs_lie_where_the_forms_change():
    assert [tf.pair_form(n) for n in tf.PAIR_RUNGS] == ["mid", "mid", "large"]
    assert tf.pair_form(tf.SMALL_MAX) == "small" and tf.pair_form(tf.SMALL_MAX + 1) == "mid"
    assert tf.pair_form(tf.MID_MAX_E64) == "mid" and tf.pair_form(tf.MID_MAX_E64 + 1) == "large"
    assert [tf.keys_form(4, n) for n in tf.KEY_RUNGS[4]] == ["mid", "large"]
    assert [tf.keys_form(8, n) for n in tf.KEY_RUNGS[8]] == ["large", "large"]
    assert tf.PAIR_RUNGS[0] > tf.SMALL_MAX and tf.PAIR_RUNGS[0] - tf.SMALL_MAX < 4096   # just past the one-workgroup sort
    assert tf.PAIR_RUNGS[2] - tf.MID_MAX_E64 < 8192 and tf.KEY_RUNGS[4][1] - tf.MID_MAX_U32 < 8192
    for n in tf.PAIR_RUNGS + tf.KEY_RUNGS[4]:
        assert n % 2 == 1 and n % 4096                                                  # odd, no multiple of a tile


def test_the_configurations_and_cases():
    assert tf.CONFIG_NAMES == ["default", "rank0", "small_partition", "one_sweep", "three_kernel_4bit"]
    assert tf.KNOBS_OF == {"default": [], "rank0": [("sort.rank", 0)], "small_partition": [("debug.resident_wgs", 120)],
                           "one_sweep": [("sort.algo", 0)], "three_kernel_4bit": [("sort.algo", 1), ("sort.digit_bits", 4)]}
    for knobs in tf.KNOBS_OF.values():
        assert all(knob in tf.RESTORE for knob, _ in knobs)
    assert tf.RESTORE["debug.resident_wgs"] == 0
    assert set(tf.CASES) >= {("f64", "normal"), ("f32", "nan30"), ("i64", "ids"), ("i64", "uniform_pm1000"), ("f64", "normal_specials")}
    for name, case in tf.CASES:
        assert case in typed_shapes.CASES[name]


def test_row_shapes_sit_on_the_rungs_with_no_power_of_two():
    for (rows, cols, stride), rung in zip(tf.ROW_SHAPES, tf.PAIR_RUNGS):
        assert tf.pair_form(rows * cols) == tf.pair_form(rung) and abs(rows * cols - rung) < 256
        assert cols & (cols - 1) and rows & (rows - 1) and stride >= cols   # ("sort.rows_algo" = 0 forces the flat path)
    assert any(stride != cols for _, cols, stride in tf.ROW_SHAPES) and any(stride == cols for _, cols, stride in tf.ROW_SHAPES)
    assert len({4 * ((int(rows - 1).bit_length() + 3) // 4) for rows, _, _ in tf.ROW_SHAPES}) == 2   # row ids of 4 and of 8 bits
    for (rows, cols, stride), rung in zip(tf.TOPK_ROW_SHAPES, tf.PAIR_RUNGS):
        assert cols == rung and rows >= 2 and stride >= cols
    assert any((stride * 8) % 16 for _, _, stride in tf.TOPK_ROW_SHAPES)   # rows of 8-byte keys that start off the 16-byte grid


def test_topk_ks():
    for n in tf.PAIR_RUNGS:
        small, large = tf.topk_ks(n)
        assert 0 < small <= n // 8 and n // 8 < large <= n
        assert tf.pair_form(large) == tf.pair_form(n)


@pytest.mark.parametrize("n,segments,longest", [(20011, 301, None), (300007, 301, None), ((1 << 20) + 4099, 301, None),
                                                 (300007, tf.PLAN_SEGMENTS, 4096), (5000, 7, 4096)])
def test_segment_lengths(n, segments, longest):
    lens = tf.segment_lengths(n, segments, 1, longest)
    assert len(lens) == segments and sum(lens) == n and min(lens) == 0
    assert lens[0] == 0 and lens[-1] == 0 and lens[segments // 2:segments // 2 + 3] == [0, 0, 0]
    live = [x for x in lens if x]
    assert len(set(live)) > min(len(live), 8) // 2, "the lengths do not vary"
    if longest is not None:
        assert max(lens) <= longest
    assert lens == tf.segment_lengths(n, segments, 1, longest)   # the same every time


def test_inner_labels_leave_the_primitives_own_kernels_out():
    labels = TYPED64 | MID3 | ROWS | {"select_hist", "segments_emit", "search_right_k32", "runs_scan", "reduce_emit_fsum_k64v64", "key_encode"}
    assert tf.inner_labels(labels) == MID3
    assert tf.inner_labels({"segments_sort_k64", "segment_sort_e64"}) == {"segment_sort_e64"}


def test_default_rules():
    pairs = [Sort("pairs", MID_N)] * 2
    tf.check_labels("default", TYPED64 | MID3, pairs)
    tf.check_labels("default", TYPED64 | PASSES8, pairs)              # sent down the per-digit passes by an earlier sort's report
    tf.check_labels("default", TYPED64 | MID3 | PASSES8, pairs)
    tf.check_labels("default", TYPED64 | LARGE_PAIRS, [Sort("pairs", TOP_N)] * 2)
    tf.check_labels("default", TYPED64 | SMALL, [Sort("pairs", 2000)] * 2)
    tf.check_labels("default", TYPED32 | MID2, [Sort("keys32", MID_N)])
    refused("default", TYPED64, pairs)                                # no inner sort at all
    refused("default", TYPED64 | SMALL, pairs)                        # a threshold moved: the rung no longer leaves the one-workgroup sort
    refused("default", TYPED64 | PASSES8, [Sort("pairs", TOP_N)] * 2)  # the large form takes every input
    refused("default", TYPED64 | MID3, [Sort("pairs", TOP_N)] * 2)
    refused("default", TYPED64 | PASSES4, pairs)
    tf.check_labels("default", {"segments_classify", "count_soa_4b", "scan_table", "scatter_soa_4b"}, [Sort("soa", 20011)])


def test_control_rules():
    tf.check_control(TYPED64 | MID3, [Sort("pairs", MID_N)] * 2)
    tf.check_control(TYPED64 | LARGE_PAIRS | SOA8 | ROWS, [Sort("pairs", TOP_N)] * 2 + [Sort("soa", TOP_N)])
    tf.check_control({"key_encode", "key_decode"} | LARGE_U32, [Sort("keys32", tf.KEY_RUNGS[4][1])])
    tf.check_control(TYPED64 | LARGE_PAIRS | PASSES8_U32, [Sort("positions", TOP_N - 5)] + [Sort("pairs", TOP_N - 5)] * 2)
    tf.check_control(TYPED64 | PASSES8 | MID2, [Sort("positions", MID_N - 5)] + [Sort("pairs", MID_N - 5)] * 2)   # (its report decided)
    for labels, sorts in ((TYPED64 | PASSES8, [Sort("pairs", MID_N)] * 2),             # the mid-size range without its form
                          (TYPED64 | MID3, [Sort("pairs", TOP_N)] * 2),                # the large rung without the large sort
                          (TYPED64 | SMALL, [Sort("pairs", 2000)] * 2),                # no rung at all
                          (TYPED64 | PASSES8 | PASSES8_U32, [Sort("positions", TOP_N - 5)] + [Sort("pairs", TOP_N - 5)] * 2),
                          (SOA8, [Sort("soa", MID_N)])):
        with pytest.raises(AssertionError):
            tf.check_control(labels, sorts)


def test_small_partition_rules():
    pairs = [Sort("pairs", TOP_N)] * 2
    tf.check_labels("small_partition", TYPED64 | PASSES8, pairs)
    tf.check_labels("small_partition", TYPED64 | SMALL, [Sort("pairs", 2000)] * 2)
    for bad in (MID3, LARGE_PAIRS, {"segment_sort_e64"}):
        refused("small_partition", TYPED64 | PASSES8 | bad, pairs)
    refused("small_partition", TYPED64 | PASSES8, pairs, net_delta=(1, 0))
    refused("small_partition", TYPED64 | PASSES8, pairs, net_delta=(0, 1))


def test_rank0_rules():
    tf.check_labels("rank0", TYPED64 | PASSES8, [Sort("pairs", MID_N)] * 2)
    tf.check_labels("rank0", TYPED64 | LARGE_PAIRS, [Sort("pairs", TOP_N)] * 2)
    tf.check_labels("rank0", TYPED64 | (LARGE_PAIRS - {"segment_sort_wave_e64"}), [Sort("pairs", TOP_N)] * 2)   # the net ran: no finish
    tf.check_labels("rank0", {"key_encode", "key_decode"} | PASSES8_U32, [Sort("keys32", tf.KEY_RUNGS[4][1])])
    refused("rank0", TYPED64 | MID3, [Sort("pairs", MID_N)] * 2)
    refused("rank0", TYPED64 | PASSES8, [Sort("pairs", TOP_N)] * 2)                     # pairs keep the stable large sort
    refused("rank0", {"key_encode", "key_decode"} | LARGE_U32, [Sort("keys32", tf.KEY_RUNGS[4][1])])   # keys leave the large form
    refused("rank0", {"key_encode"} | {"msd2s_prep", "msd2s_pass1_u64", "msd2s_pass2_u64", "msd2s_offsets"}, [Sort("keys64", MID_N)])


def test_one_sweep_rules():
    pairs = [Sort("pairs", MID_N)] * 2
    tf.check_labels("one_sweep", TYPED64 | ONE_SWEEP, pairs)
    tf.check_labels("one_sweep", TYPED64 | ROWS | ONE_SWEEP | {"os_hist_u32", "onesweep_soa_8b"}, pairs + [Sort("soa", MID_N)])
    refused("one_sweep", TYPED64 | MID3, pairs)               # (the mid-size form has a onesweep_ label of its own)
    refused("one_sweep", TYPED64 | ONE_SWEEP | SMALL, pairs)
    refused("one_sweep", TYPED64 | ONE_SWEEP | PASSES8, pairs)
    refused("one_sweep", TYPED64 | PASSES8, pairs)


def test_three_kernel_4bit_rules():
    pairs = [Sort("pairs", MID_N)] * 2
    tf.check_labels("three_kernel_4bit", TYPED64 | PASSES4, pairs)
    tf.check_labels("three_kernel_4bit", TYPED64 | PASSES4 | {"count_soa_4b", "scatter_soa_4b"}, pairs + [Sort("soa", MID_N)])
    refused("three_kernel_4bit", TYPED64 | PASSES4 | {"scatter_e64_8b"}, pairs)
    refused("three_kernel_4bit", TYPED64 | PASSES8, pairs)
    refused("three_kernel_4bit", TYPED64 | {"count_e64_4b", "scan_table"}, pairs)
    refused("three_kernel_4bit", TYPED64 | PASSES4 | SMALL, pairs)


def test_expected_results_are_computed_once():
    once = tf.Once()
    made = []
    for _ in tf.CONFIG_NAMES:
        got = once.get(("perm", "f64", "normal", 20011, 0), lambda: made.append(1) or np.arange(3))
    assert len(made) == 1 and once.computed == 1 and np.array_equal(got, np.arange(3))
