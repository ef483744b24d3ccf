"""statmc_accumulate_records_split / statmc_accumulate_records_interleaved_split without a GPU: the symbols and their
declarations, the Python keyword, what the entries answer without a device, and the chunk rule -- records_split_chunk of
statmc_amd/csrc/statmc_records_plan.h, printed by tests/cpp/test_records_split_plan.cpp (which compiles that header alone: no
library, no device; once more under AddressSanitizer and UBSan) and compared with a numpy restatement of include/statmc.h."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "test_records_split_plan.cpp")
COUNTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 2 ** 24 - 1, 2 ** 31 - 1]
LANES = 64


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def test_symbols_are_exported_and_declared(lib):
    from statmc_amd import api
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    want = {
        "statmc_accumulate_records_split": "uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, "
                                           "const int32_t *pixels, int64_t n_records, int32_t split_above, void *stream",
        "statmc_accumulate_records_interleaved_split": "uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, "
                                                       "const void *records, const statmc_record_layout *layout, int64_t n_records, "
                                                       "int32_t split_above, void *stream",
    }
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, "include/statmc.h does not declare %s" % name
        assert " ".join(decl.group(1).split()) == args
    assert re.search(r"#define\s+STATMC_RECORDS_SPLIT_LANES\s+64\b", header)
    default = re.search(r"#define\s+STATMC_RECORDS_SPLIT_DEFAULT\s+(\d+)\b", header)
    assert default and int(default.group(1)) >= 1
    assert api.RECORDS_SPLIT_LANES == 64 and api.RECORDS_SPLIT_DEFAULT == int(default.group(1))
    # the existing entries keep their argument lists: split_above is a keyword that defaults to the sequential entry
    for f in (api.accumulate_records, api.accumulate_records_interleaved):
        assert inspect.signature(f).parameters["split_above"].default is None


def _types(api, kinds):
    arr = (api.StatType * 16)()
    for i, (c, t, m) in enumerate(kinds):
        arr[i].channels, arr[i].transform, arr[i].max_moment = c, t, m
    return arr


def test_without_a_device_the_entries_return_an_error(lib):
    """Made-up pointers, never dereferenced.  split_above < 1 is refused with the argument named whether or not a device is set
    up; the limits of the sequential entries come first, as there; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    types = _types(api, [(3, 1, 3), (1, 0, 1)])
    lay = api.make_record_layout(20, 0, [4, 16])
    per_array = lambda n_types=2, n=100, k=8: lib.statmc_accumulate_records_split(8, 8, types, n_types, 0x10000, n, k, None)
    interleaved = lambda n_types=2, n=100, k=8: lib.statmc_accumulate_records_interleaved_split(8, 8, types, n_types, 0x10000, C.byref(lay), n, k, None)
    for call in (per_array, interleaved):
        for k in (0, -1, -2 ** 31):
            assert call(k=k) == api.ERR_INVALID
            assert b"split_above" in lib.statmc_last_error()
        assert call(n=-1) == api.ERR_INVALID and b"n_records" in lib.statmc_last_error()
        assert call(n=2 ** 31, k=0) == api.ERR_INVALID and b"n_records" in lib.statmc_last_error()      # the existing order of checks
        assert call(n_types=17) == api.ERR_INVALID and b"n_types" in lib.statmc_last_error()
    bad = api.make_record_layout(18, 0, [4, 16])
    assert lib.statmc_accumulate_records_interleaved_split(8, 8, types, 2, 0x10000, C.byref(bad), 100, 8, None) == api.ERR_INVALID
    assert b"stride" in lib.statmc_last_error()
    if torch.cuda.is_available():       # the valid calls would run on made-up pointers (tests/test_records_split_gpu.py runs real ones)
        return
    for call in (per_array, interleaved):
        for k in (1, 8, 2 ** 31 - 1):
            assert call(k=k) == api.ERR_NO_DEVICE
        assert call(n=0) == api.ERR_NO_DEVICE and call(n_types=0) == api.ERR_NO_DEVICE       # a no-op only after setup


def chunks_of(cnt):
    """include/statmc.h restated: L = ceil(cnt / 64), slot j owns [min(j L, cnt), min((j + 1) L, cnt))"""
    L = -(-cnt // LANES)
    j = np.arange(LANES, dtype=np.int64)
    lo, hi = np.minimum(j * L, cnt), np.minimum((j + 1) * L, cnt)
    return lo, hi - lo


def _run(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


@pytest.fixture(scope="module")
def plan_out():
    from statmc_amd import build
    build.build_tools()
    return _run(build.REC_SPLIT_PLAN_BIN).stdout


def test_the_chunk_rule(plan_out):
    got = {}
    for line in plan_out.splitlines():
        name, _, rest = line.partition(" : ")
        if name.startswith("chunks "):
            got[int(name.split()[1])] = np.array(rest.split(), dtype=np.int64).reshape(LANES, 2)
    assert sorted(got) == COUNTS
    for cnt in COUNTS:
        begin, length = got[cnt][:, 0], got[cnt][:, 1]
        lo, ln = chunks_of(cnt)
        assert np.array_equal(begin, lo) and np.array_equal(length, ln), cnt
        # the chunks tile [0, cnt) in slot order: each starts where the one before it ends, none is negative, no chunk follows an
        # empty one, and every chunk but the last non-empty one has the full length
        assert begin[0] == 0 and (length >= 0).all() and begin[-1] + length[-1] == cnt
        assert np.array_equal(begin[1:], (begin + length)[:-1])
        full = -(-cnt // LANES)
        nonempty = int((length > 0).sum())
        assert (length[:max(nonempty - 1, 0)] == full).all() and (length[nonempty:] == 0).all()
        assert cnt == 0 or 0 < length[nonempty - 1] <= full


def test_the_threshold_check(plan_out):
    got = dict(line.partition(" : ")[::2] for line in plan_out.splitlines() if line.startswith("split_above "))
    assert sorted(int(k.split()[1]) for k in got) == sorted([-2 ** 31, -1, 0, 1, 8, 2 ** 31 - 1] + [int(re.search(
        r"#define\s+STATMC_RECORDS_SPLIT_DEFAULT\s+(\d+)", open(os.path.join(ROOT, "include", "statmc.h")).read()).group(1))])
    for k, v in got.items():
        if int(k.split()[1]) >= 1:
            assert v == "ok", (k, v)
        else:
            assert v != "ok" and "split_above" in v, (k, v)


def test_the_plan_program_is_clean_under_sanitizers(plan_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own:
    no report, the same lines."""
    binary = str(tmp_path / "split_plan_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), PLAN_SRC, "-o", binary])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout == plan_out
