"""oclradixsort_amd/csrc/large_plan.hpp on the CPU: the plan of a large sort -- form, head-room, 16-bit second slab, binning finish,
layout -- and the large sort's term of the scratch query, against the Python twins of tests/large_plan.py.

tests/large_plan_dump.cpp (the header and a main, no HIP call, nothing linked) is compiled with the host compiler and prints one
row per case.  The twins restate the capacities and the decisions; the byte offsets are not restated: the chain's twin is fed the
totals the header's own layouts report.  No GPU.
"""
import itertools
import os
import shutil
import subprocess
from functools import lru_cache
from pathlib import Path

import pytest

import large_plan as lp
from large_plan import KV32, MI, SOA32, U32, U64

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "oclradixsort_amd" / "csrc"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

MAX_ELEMS = 0xFFF00000          # kMaxElems (adlhip_internal.hpp)
KINDS = [U32, KV32, U64, SOA32]
SORT_BITS = ["whole", 28, 16, 12]
MSD2 = [0, 1, 2, 3, 4, 5]
OFFERED = ["l0", "l2", "l1", "m02", "m21"]
# every size at which some decision of the header changes, with its neighbours: kSmallMax = kMsd2Min; kMsd2sAutoMin; kMsd2AutoMin;
# kSlabInTmpMin = the end of the narrow second digit (seg_shift reaches 8); the binning finish and its form (24, 48 Mi); the hybrid
# form without and with the persistent passes, and "sort.rank" = 0 (96, 192 Mi); kMsd2sMax = kMsd2MaxU64; the last wave-sized tile
# (280 Mi); kMsd2MaxU32; the largest n the library takes
EDGES = [16384, MI, 2 * MI, 16 * MI, 24 * MI, 48 * MI, 96 * MI, 192 * MI, 256 * MI + 4 * MI, 280 * MI, 1088 * MI]
NS = sorted({e + k for e in EDGES for k in (-1, 0, 1)} | {MAX_ELEMS - 1, MAX_ELEMS})


def _bits(kind, b):
    return (64 if kind == U64 else 32) if b == "whole" else b


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """every case through the compiled header, once: {case tuple: {name: value}}"""
    exe = tmp_path_factory.mktemp("large_plan") / "large_plan_dump"
    cxx = shutil.which("g++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")   # any host compiler does
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                        "-I", str(CSRC), str(ROOT / "tests" / "large_plan_dump.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = [(kind, _bits(kind, b), msd2, rank, persist, resident, n, offered)
             for kind, b, msd2, rank, persist, resident, n, offered
             in itertools.product(KINDS, SORT_BITS, MSD2, (0, 1), (0, 1), (120, 256), NS, OFFERED)]
    text = "".join("%d %d %d %d %d %d %d %s\n" % c for c in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        case = tuple(int(x) for x in f[:7]) + (f[7],)
        out[case] = {k: (v if k in ("preferred", "form") else int(v)) for k, v in (x.split("=") for x in f[8:])}
    assert list(out) == cases   # every case answered, in order
    return out


@lru_cache(maxsize=None)
def _twin_layout(kind, n, bits, form, lean):
    return lp.layout_of(kind, n, bits, form, lean)


def _totals(row):
    return {("cursor", False): row["cursor_full"], ("cursor", True): row["cursor_lean"],
            ("stable", False): row["stable_full"], ("stable", True): row["stable_lean"]}


def test_the_grid_covers_the_issue():
    assert len(NS) == 3 * len(EDGES) + 2 and MAX_ELEMS in NS
    assert {lp.SMALL_MAX, lp.STABLE_MAX, lp.CURSOR_MAX[4], lp.CURSOR_MAX[8], lp.SLAB_IN_TMP_MIN} <= set(EDGES)


def test_layouts_exist_exactly_where_the_shared_conditions_say(rows):
    for (kind, bits, msd2, rank, persist, resident, n, offered), row in rows.items():
        eb, whole = lp.elem_bytes_of(kind), lp.is_whole(kind, bits)
        co, so = lp.cursor_eligible(eb, kind in (U32, U64), whole, n), lp.stable_eligible(n)
        assert (row["cursor_full"] >= 0, row["cursor_lean"] >= 0, row["stable_full"] >= 0, row["stable_lean"] >= 0) == (co, co, so, so)
        if co:
            assert 0 < row["cursor_lean"] <= row["cursor_full"]
        if so:
            assert 0 < row["stable_lean"] <= row["stable_full"]


def test_the_plan_is_the_twins_plan(rows):
    for case, row in rows.items():
        kind, bits, msd2, rank, persist, resident, n, offered = case
        preferred = lp.large_sort_form(kind, n, bits, msd2, rank, persist, resident)
        assert row["preferred"] == (preferred or "none"), case
        form, lean, headroom = lp.choose(preferred, lp.large_fallbacks(kind, n, bits), _totals(row), row["offered"])
        assert (row["form"], row["lean"], row["headroom"]) == (form or "none", int(lean), headroom), case
        if form is None:
            assert row["total"] == row["work_bytes"] == 0, case
            continue
        L = _twin_layout(kind, n, bits, form, lean)
        for name in ("seg_shift", "stride_a", "stride_b", "tier_b"):
            assert row[name] == L[name], (case, name)
        assert (row["pieces"], row["slice"]) == ((0, 0) if form == "cursor" else (L["pieces"], L["slice"])), case
        assert (row["tiles_per_bucket"] > 0) == (form == "cursor"), case
        assert row["slab16"] == int(lp.plan_slab16(kind, bits, L)), case
        assert row["slab_b_in_tmp"] == int(lp.slab_b_in_tmp(kind, n, bits, L)), case
        assert row["bin"] == int(lp.bin_finish(kind, n, bits, L)), case
        assert row["total"] == row["work_bytes"] == _totals(row)[("cursor" if form == "cursor" else "stable", lean)], case
        assert row["work_bytes"] <= row["offered"], case


def test_the_scratch_term_walks_the_same_candidates(rows):
    for case, row in rows.items():
        kind, bits, msd2, rank, persist, resident, n, offered = case
        for level in (1, 2):
            assert row["l%d" % level] == lp.large_work_bytes_at(kind, n, bits, level, _totals(row)), (case, level)
        assert row["l2"] <= row["l1"], case


def test_the_scratch_levels_keep_their_promise(rows):
    """Level 1 holds whatever form the knobs prefer at full head-room; level 2 still holds a large sort wherever level 1 does; and a
    buffer of exactly a plan's work_bytes yields that plan again."""
    seen = set()
    for case, row in rows.items():
        kind, bits, msd2, rank, persist, resident, n, offered = case
        assert row["again"] == 1, case
        if row["preferred"] == "none":
            assert row["form"] == "none", case
            continue
        if offered == "l1":
            assert (row["form"], row["lean"]) == (row["preferred"], 0), case
        if offered == "l2":
            assert row["form"] != "none", case
        if offered == "l0":
            assert row["form"] == "none", case
        seen.add((row["form"], row["lean"], row["headroom"]))
    assert seen == {("none", 0, 50), ("cursor", 0, 50), ("cursor", 1, 12), ("stable", 0, 50), ("stable", 1, 50), ("hybrid", 0, 50)}
