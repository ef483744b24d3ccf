"""statmc_accumulate_formats without a GPU: the symbol, its declaration, the Python entry and constants, and the argument checks,
which are reported before anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def stat_types(api, n, samples=0x1000):
    """Descriptors that pass every host-side check (no call below gets as far as reading through them)."""
    types = (api.StatType * max(n, 1))()
    for t in types:
        t.channels, t.transform, t.max_moment, t.n_samples = 3, 0, 1, 1
        t.samples, t.n, t.mean = samples, 0x2000, 0x3000
    return types


def formats(*f):
    return (C.c_int32 * max(len(f), 1))(*f)


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "statmc_accumulate_formats")
    assert hasattr(lib, "statmc_debug_last_accumulate_loader")
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decl = re.search(r"int\s+statmc_accumulate_formats\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/statmc.h does not declare statmc_accumulate_formats"
    args = " ".join(decl.group(1).split())
    assert args == ("uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats, "
                    "int n_types, const int32_t *ranges, int n_ranges, void *stream")
    assert re.search(r"#define\s+STATMC_SAMPLES_F32\s+0\b", header) and re.search(r"#define\s+STATMC_SAMPLES_F16\s+1\b", header)
    debug = open(os.path.join(ROOT, "include", "statmc_debug.h")).read()
    assert re.search(r"int\s+statmc_debug_last_accumulate_loader\s*\(\s*void\s*\)\s*;", debug)
    assert lib.statmc_version() == 101


def test_python_entry_and_constants_exist():
    import inspect
    from statmc_amd import api
    assert (api.SAMPLES_F32, api.SAMPLES_F16) == (0, 1)
    assert "sample_formats" in inspect.signature(api.accumulate).parameters
    assert "statmc_accumulate_formats" in api.EXPORTS
    assert callable(api.last_accumulate_loader)


@pytest.mark.parametrize("bad", [2, -1])
def test_unknown_formats_are_refused_before_any_device_work(lib, bad):
    from statmc_amd import api
    types = stat_types(api, 2)
    for fmts in (formats(bad, 0), formats(1, bad), formats(0, bad)):
        assert lib.statmc_accumulate_formats(8, 8, types, fmts, 2, None, 0, None) == api.ERR_INVALID
        assert b"sample_formats" in lib.statmc_last_error()


def test_limits_are_refused_before_any_device_work(lib):
    from statmc_amd import api
    types = stat_types(api, 17)
    half = formats(*([1] * 17))
    assert lib.statmc_accumulate_formats(8, 8, types, half, 17, None, 0, None) == api.ERR_INVALID
    assert b"n_types" in lib.statmc_last_error()
    assert lib.statmc_accumulate_formats(8, 8, types, half, -1, None, 0, None) == api.ERR_INVALID
    assert b"n_types" in lib.statmc_last_error()
    ranges = (C.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    assert lib.statmc_accumulate_formats(8, 8, types, half, 6, ranges, 3, None) == api.ERR_INVALID     # 18 > 16
    assert lib.statmc_accumulate_formats(8, 8, types, half, 2, ranges, -1, None) == api.ERR_INVALID


def test_an_odd_arena_address_is_refused_before_any_device_work(lib):
    from statmc_amd import api
    types = stat_types(api, 2, samples=0x1001)
    assert lib.statmc_accumulate_formats(8, 8, types, formats(0, 1), 2, None, 0, None) == api.ERR_INVALID
    assert b"odd address" in lib.statmc_last_error()


def test_refuses_to_run_before_setup(lib):
    """In a process that has set a device up (a GPU is present) the order of the suite decides whether this process is still
    "before setup", so the check is made where no device can have been set up."""
    import torch
    from statmc_amd import api
    if not torch.cuda.is_available():
        types = stat_types(api, 2)
        for fmts in (formats(1, 1), formats(0, 1), formats(0, 0), None):
            assert lib.statmc_accumulate_formats(8, 8, types, fmts, 2, None, 0, None) == api.ERR_NO_DEVICE
        ranges = (C.c_int32 * 2)(1, 3)
        assert lib.statmc_accumulate_formats(8, 8, types, formats(1, 1), 2, ranges, 1, None) == api.ERR_NO_DEVICE
        assert lib.statmc_debug_last_accumulate_loader() == 0
