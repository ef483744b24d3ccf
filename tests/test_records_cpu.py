"""statmc_accumulate_records without a GPU: the symbol, its declaration, the Python entry, and the argument limits, which are
reported before anything touches a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "statmc_accumulate_records")
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decl = re.search(r"int\s+statmc_accumulate_records\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/statmc.h does not declare statmc_accumulate_records"
    args = " ".join(decl.group(1).split())
    assert args == ("uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, "
                    "const int32_t *pixels, int64_t n_records, void *stream")


def test_python_entry_exists():
    from statmc_amd import api
    assert callable(api.accumulate_records)
    assert callable(api.make_stat_type_records)


def test_limits_are_refused_before_any_device_work(lib):
    from statmc_amd import api
    types = (api.StatType * 17)()
    for n_records in (-1, 2 ** 31, 2 ** 40):
        assert lib.statmc_accumulate_records(8, 8, types, 1, None, n_records, None) == api.ERR_INVALID, n_records
        assert b"n_records" in lib.statmc_last_error()
    assert lib.statmc_accumulate_records(8, 8, types, 17, None, 4, None) == api.ERR_INVALID
    assert lib.statmc_accumulate_records(8, 8, types, -1, None, 4, None) == api.ERR_INVALID
    assert b"n_types" in lib.statmc_last_error()


def test_refuses_to_run_before_setup(lib):
    """Like every compute entry; in a process that has set a device up (a GPU is present) the order of the suite decides
    whether this process is still "before setup", so the check is made where no device can have been set up."""
    import torch
    from statmc_amd import api
    if not torch.cuda.is_available():
        types = (api.StatType * 1)()
        assert lib.statmc_accumulate_records(8, 8, types, 1, None, 4, None) == api.ERR_NO_DEVICE
        assert lib.statmc_accumulate_records(8, 8, None, 0, None, 0, None) == api.ERR_NO_DEVICE   # a no-op only after setup
        assert lib.statmc_debug_accumulate_records_phases(3) == api.ERR_NO_DEVICE
    assert lib.statmc_debug_accumulate_records_phases(0) == api.ERR_INVALID
    assert lib.statmc_debug_accumulate_records_phases(4) == api.ERR_INVALID
