"""Typed keys, order and argsort: what can be checked without a GPU (the C ABI's refusals, the facade's host path and its exported
symbols), plus the facade's device path on the GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from oclradixsort_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEMO = os.path.join(ROOT, "tests", "demo", "typed_demo")
FACADE = os.path.join(ROOT, "oclradixsort_amd", "lib", "libtahoe_pprims.so")


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(DEMO) and os.path.exists(FACADE)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_null_handle_is_rejected_by_the_typed_entry_points(built):
    lib = built
    sz = ctypes.c_size_t()
    calls = {
        "adlhip_key_encode": lambda: lib.adlhip_key_encode(None, 2, 0, None, None, 16),
        "adlhip_key_decode": lambda: lib.adlhip_key_decode(None, 2, 0, None, None, 16),
        "adlhip_sort_typed_scratch_bytes": lambda: lib.adlhip_sort_typed_scratch_bytes(None, 2, 0, 0, 1024, ctypes.byref(sz),
                                                                                       ctypes.byref(sz), ctypes.byref(sz)),
        "adlhip_sort_keys_typed": lambda: lib.adlhip_sort_keys_typed(None, 2, 0, None, None, None, 0, 16),
        "adlhip_sort_pairs_typed": lambda: lib.adlhip_sort_pairs_typed(None, 2, 0, None, None, 4, None, None, None, 0, 16),
        "adlhip_argsort_typed": lambda: lib.adlhip_argsort_typed(None, 2, 0, None, None, None, None, 0, 16),
    }
    for name, call in calls.items():
        assert call() == 1, name   # ADLHIP_FAILURE
        assert b"null device handle" in lib.adlhip_last_error(), name


def test_typed_names_are_bound_with_the_headers_values():
    header = open(os.path.join(ROOT, "include", "adlhip.h")).read()
    values = dict(re.findall(r"#define (ADLHIP_(?:KEY|ORDER)_[A-Z0-9]+)\s+(\d+)", header))
    assert values == {"ADLHIP_KEY_U32": "0", "ADLHIP_KEY_I32": "1", "ADLHIP_KEY_F32": "2", "ADLHIP_KEY_U64": "3",
                      "ADLHIP_KEY_I64": "4", "ADLHIP_KEY_F64": "5", "ADLHIP_ORDER_ASCENDING": "0", "ADLHIP_ORDER_DESCENDING": "1"}
    import numpy as np
    from oclradixsort_amd import pprims
    assert {np.dtype(k).name: v for k, v in pprims.KEY_TYPES.items()} == {
        "uint32": 0, "int32": 1, "float32": 2, "uint64": 3, "int64": 4, "float64": 5}
    for name in ("adlhip_key_encode", "adlhip_key_decode", "adlhip_sort_typed_scratch_bytes", "adlhip_sort_keys_typed",
                 "adlhip_sort_pairs_typed", "adlhip_argsort_typed"):
        assert name in _lib.SIGNATURES


def test_torch_sorter_is_exported_lazily():
    import oclradixsort_amd
    assert "TorchSorter" not in vars(oclradixsort_amd) or callable(oclradixsort_amd.TorchSorter)
    from oclradixsort_amd import TorchSorter
    assert TorchSorter.__name__ == "TorchSorter" and callable(TorchSorter.sort) and callable(TorchSorter.argsort)
    with pytest.raises(AttributeError):
        oclradixsort_amd.NoSuchName


def _demo_lines(args):
    r = subprocess.run([DEMO] + args, capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return lines


def _check_demo(lines):
    assert len(lines) == 24, lines   # six types x two orders x two sizes
    assert all(ln.startswith("[ OK ] Typed.") for ln in lines), [ln for ln in lines if not ln.startswith("[ OK ]")]
    for t in ("u32", "i32", "f32", "u64", "i64", "f64"):
        for o in ("ascending", "descending"):
            assert sum(("Typed.%s %s " % (t, o)) in ln for ln in lines) == 2, (t, o)


def test_typed_demo_host_path(built):
    _check_demo(_demo_lines(["--host"]))


def test_facade_exports_the_typed_methods(built):
    out = subprocess.run(["nm", "-DC", "--defined-only", FACADE], capture_output=True, text=True).stdout
    for t in ("int", "float", "long long", "double", "unsigned int", "unsigned long long"):
        assert re.search(r" T Tahoe::Pprims::sortKeys\(adl::Device const\*, adl::Buffer<%s> const&, int, bool\)" % re.escape(t), out), t
        assert re.search(r" T Tahoe::Pprims::argsort\(adl::Device const\*, adl::Buffer<%s> const&, adl::Buffer<unsigned int>&, int, bool\)"
                         % re.escape(t), out), t


@pytest.mark.gpu
def test_typed_demo_device_path(built):
    _check_demo(_demo_lines([]))
