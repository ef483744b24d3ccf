"""statmc_accumulate_records_interleaved without a GPU: the symbol and its declaration, the Python entries, every argument rule
of include/statmc.h -- refused with the argument named before anything touches a device -- and the fold that
statmc::plan_records_interleaved picks (tests/cpp/test_records_interleaved_plan.cpp, which compiles
statmc_amd/csrc/statmc_records_plan.h alone: no library, no device; once more under AddressSanitizer and UBSan)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SRC = os.path.join(ROOT, "tests", "cpp", "test_records_interleaved_plan.cpp")


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def test_symbol_is_exported_and_declared(lib):
    assert hasattr(lib, "statmc_accumulate_records_interleaved")
    assert hasattr(lib, "statmc_debug_accumulate_records_interleaved_path")
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decl = re.search(r"int\s+statmc_accumulate_records_interleaved\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/statmc.h does not declare statmc_accumulate_records_interleaved"
    assert " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, "
                                               "const void *records, const statmc_record_layout *layout, int64_t n_records, void *stream")
    struct = re.search(r"typedef struct statmc_record_layout \{(.*?)\} statmc_record_layout;", header, re.S)
    assert struct, "include/statmc.h does not define statmc_record_layout"
    fields = [" ".join(f.split()) for f in re.sub(r"/\*.*?\*/", "", struct.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == ["int32_t stride", "int32_t pixel_offset", "int32_t sample_offset[16]", "int32_t sample_format[16]"]
    debug = open(os.path.join(ROOT, "include", "statmc_debug.h")).read()
    assert re.search(r"int\s+statmc_debug_accumulate_records_interleaved_path\s*\(\s*int\s+\w+\s*\)\s*;", debug)


def test_python_entries_exist_and_mirror_the_struct():
    from statmc_amd import api
    assert callable(api.accumulate_records_interleaved)
    assert callable(api.make_record_layout) and callable(api.pack_records) and callable(api.make_stat_type_record_field)
    assert callable(api.accumulate_records_interleaved_path) and callable(api.last_accumulate_records_interleaved_path)
    assert "statmc_accumulate_records_interleaved" in api.EXPORTS
    lay = api.RecordLayout
    assert C.sizeof(lay) == 4 * 34
    assert (lay.stride.offset, lay.pixel_offset.offset, lay.sample_offset.offset, lay.sample_format.offset) == (0, 4, 8, 72)


def test_pack_records_lays_the_fields_out_as_the_layout_says():
    from statmc_amd import api
    px = np.array([5, -1, 7], np.int32)
    rad = np.arange(9, dtype=np.float32).reshape(3, 3) + 0.5
    depth = np.array([1.0, 2.0, 65504.0], np.float32)
    rec, lay = api.pack_records(px, [rad, depth], formats=[api.SAMPLES_F32, api.SAMPLES_F16])
    assert (lay.stride, lay.pixel_offset, lay.sample_offset[0], lay.sample_offset[1]) == (20, 0, 4, 16)
    assert (lay.sample_format[0], lay.sample_format[1]) == (api.SAMPLES_F32, api.SAMPLES_F16)
    rows = rec.reshape(3, 20)
    assert np.array_equal(rows[:, 0:4].copy().view(np.int32).reshape(-1), px)
    assert np.array_equal(rows[:, 4:16].copy().view(np.float32), rad)
    assert np.array_equal(rows[:, 16:18].copy().view(np.float16).reshape(-1), depth.astype(np.float16))
    assert not rows[:, 18:].any()
    # the pixel in the middle, the fields in reversed order, padding that holds the fill byte
    rec, lay = api.pack_records(px, [rad, depth], stride=32, pixel_offset=12, offsets=[16, 4], fill=0xAB)
    rows = rec.reshape(3, 32)
    assert np.array_equal(rows[:, 12:16].copy().view(np.int32).reshape(-1), px)
    assert np.array_equal(rows[:, 16:28].copy().view(np.float32), rad)
    assert np.array_equal(rows[:, 4:8].copy().view(np.float32).reshape(-1), depth)
    assert (rows[:, 0:4] == 0xAB).all() and (rows[:, 8:12] == 0xAB).all() and (rows[:, 28:] == 0xAB).all()
    with pytest.raises(ValueError):
        api.pack_records(px, [rad], stride=12)


def _types(api, kinds):
    arr = (api.StatType * 17)()
    for i, (c, t, m) in enumerate(kinds):
        arr[i].channels, arr[i].transform, arr[i].max_moment = c, t, m
    return arr


FIVE = [(3, 1, 3), (3, 0, 1), (3, 0, 1), (1, 0, 1), (1, 0, 1)]
FIVE_OFFSETS = [4, 16, 28, 40, 44]


def test_every_invalid_argument_is_refused_before_any_device_work(lib):
    """Through the C entry itself; the pointers are made up and never dereferenced.  Where no GPU is present no device can have
    been set up, so anything the entry let through would come back as STATMC_ERR_NO_DEVICE, not STATMC_ERR_INVALID."""
    from statmc_amd import api
    types = _types(api, FIVE)
    f = lib.statmc_accumulate_records_interleaved
    REC = 0x10000

    def refused(what, n_types=5, records=REC, n_records=100, layout="ok", **change):
        if layout == "ok":
            layout = api.make_record_layout(48, 0, FIVE_OFFSETS)
            for k, v in change.items():
                if isinstance(v, tuple):
                    getattr(layout, k)[v[0]] = v[1]
                else:
                    setattr(layout, k, v)
        rc = f(8, 8, types, n_types, records, C.byref(layout) if layout is not None else None, n_records, None)
        assert rc == api.ERR_INVALID, (what, rc)
        assert what.encode() in lib.statmc_last_error(), (what, lib.statmc_last_error())

    for n in (-1, 2 ** 31, 2 ** 40):
        refused("n_records", n_records=n)
    refused("n_types", n_types=17)
    refused("n_types", n_types=-1)
    refused("layout", layout=None)                         # types and records to work on, no layout
    refused("layout", layout=None, n_types=0)              # ... records only
    refused("layout", layout=None, n_records=0)            # ... types only
    for stride in (0, 2, -48, 50, 46):
        refused("stride", stride=stride)
    for records in (REC + 1, REC + 2, REC + 3):
        refused("records", records=records)
    for off in (-4, 2, 6, 46, 48, 2 ** 31 - 4):
        refused("pixel_offset", pixel_offset=off)
    for off in (-4, -1, 6, 18, 40, 48, 2 ** 31 - 4):       # negative, not a multiple of 4, the RGB field's end behind the stride
        refused("sample_offset[1]", sample_offset=(1, off))
    refused("sample_offset[4]", sample_offset=(4, 48))     # a 1-channel fp32 field that starts at the stride
    refused("sample_offset[4]", sample_offset=(4, 46))
    for fmt in (-1, 2, 16):
        refused("sample_format[3]", sample_format=(3, fmt))
    # a half field: any multiple of 2 whose 2 C bytes fit; odd offsets and an end behind the stride do not
    lay = api.make_record_layout(48, 0, FIVE_OFFSETS, [api.SAMPLES_F32, api.SAMPLES_F16, api.SAMPLES_F32, api.SAMPLES_F16, api.SAMPLES_F32])
    for t, off in ((1, 7), (1, 44), (1, -2), (3, 48), (3, 47)):
        bad = api.RecordLayout.from_buffer_copy(lay)
        bad.sample_offset[t] = off
        refused("sample_offset[%d]" % t, layout=bad)
    types[2].channels = 2
    refused("types[2]")


def test_valid_calls_get_as_far_as_the_device(lib):
    """The other side of every rule: the largest and oddest valid arguments pass the checks.  Without a GPU that shows as
    STATMC_ERR_NO_DEVICE (also for the no-ops: a no-op only after setup, like statmc_accumulate_records)."""
    import torch
    from statmc_amd import api
    if torch.cuda.is_available():       # the calls would run on made-up pointers (tests/test_records_interleaved_gpu.py runs real ones)
        return
    types = _types(api, FIVE)
    f = lib.statmc_accumulate_records_interleaved
    ok = api.make_record_layout(48, 0, FIVE_OFFSETS)
    assert f(8, 8, types, 5, 0x10000, C.byref(ok), 100, None) == api.ERR_NO_DEVICE
    assert f(8, 8, types, 5, 0x10004, C.byref(ok), 2 ** 31 - 1, None) == api.ERR_NO_DEVICE
    assert f(8, 8, None, 0, None, None, 0, None) == api.ERR_NO_DEVICE
    assert f(8, 8, _types(api, [(1, 0, 1)] * 16), 16, 0x10000, C.byref(api.make_record_layout(4, 0, [0] * 16)), 5, None) == api.ERR_NO_DEVICE   # every field on the pixel
    lay = api.make_record_layout(52, 48, [36, 24, 6, 2, 46], [api.SAMPLES_F32, api.SAMPLES_F32, api.SAMPLES_F16, api.SAMPLES_F16, api.SAMPLES_F16])
    assert f(8, 8, types, 5, 0x10000, C.byref(lay), 5, None) == api.ERR_NO_DEVICE
    assert lib.statmc_debug_accumulate_records_interleaved_path(1) == api.ERR_NO_DEVICE


def test_debug_path_values(lib):
    from statmc_amd import api
    assert lib.statmc_debug_accumulate_records_interleaved_path(-1) == api.ERR_INVALID
    assert lib.statmc_debug_accumulate_records_interleaved_path(3) == api.ERR_INVALID
    assert b"statmc_debug_accumulate_records_interleaved_path" in lib.statmc_last_error()


def _run_plan(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for line in out.stdout.splitlines():
        name, _, rest = line.partition(" : ")
        assert name not in got, name
        got[name] = rest
    return got, out.stdout


@pytest.fixture(scope="module")
def plan_lines():
    from statmc_amd import build
    build.build_tools()
    return _run_plan(build.REC_ILV_PLAN_BIN)


GENERAL = "1 0 0 0"


def test_the_path_chosen(plan_lines):
    """path K M fmt, then the fused slots' type indices (radiance, the RGB types, the 1-channel types)."""
    got, _ = plan_lines
    want = {
        # the shipped 11-channel set: fused, in each of its format classes; other mixes of formats are the general fold's
        "plan five f32": "2 2 2 0 0 1 2 3 4",
        "plan five feat16": "2 2 2 1 0 1 2 3 4",
        "plan five all16": "2 2 2 2 0 1 2 3 4",
        "plan five rad16 only": GENERAL,
        "plan five mixed features": GENERAL,
        "plan five f32 forced general": GENERAL,
        "plan five f32 forced fused": "2 2 2 0 0 1 2 3 4",
        "plan five shuffled types": "2 2 2 0 2 1 4 0 3",
        "plan three": "2 2 0 0 0 1 2",
        "plan rad+f1": "2 0 1 0 0 1",
        # one type, sixteen types, and sets outside the fused classes: general, also when fused is asked for
        "plan one type": GENERAL,
        "plan one type forced fused": GENERAL,
        "plan sixteen": GENERAL,
        "plan sixteen forced fused": GENERAL,
        "plan features only": GENERAL,
        "plan two radiance": GENERAL,
        "plan three rgb": GENERAL,
        "plan tests' four": GENERAL,
        # overlapping fields change nothing: the type set decides
        "plan overlap rad+rgb+f1": "2 1 1 0 0 1 2",
        "plan overlap two radiance": GENERAL,
    }
    assert {k: v for k, v in got.items() if k.startswith("plan ")} == want


def test_the_layout_rules(plan_lines):
    got, _ = plan_lines
    checks = {k[len("check "):]: v for k, v in got.items() if k.startswith("check ")}
    valid = ["tight 48", "n_records 2^31 - 1", "null layout, nothing to do", "records + 4", "stride 4, no types", "pixel_offset 44",
             "rgb f32 at 36 of 48", "half offset 6", "rgb half at 42 of 48", "garbage behind n_types"]
    named = {"n_types 17": "n_types", "n_types -1": "n_types", "n_records -1": "n_records", "n_records 2^31": "n_records",
             "null layout, records": "layout", "null layout, types": "layout", "null types": "types", "records + 2": "records",
             "stride 0": "stride", "stride -48": "stride", "stride 50": "stride", "pixel_offset -4": "pixel_offset",
             "pixel_offset 2": "pixel_offset", "pixel_offset 48": "pixel_offset", "offset -4": "sample_offset[1]",
             "f32 offset 6": "sample_offset[1]", "rgb f32 at 40 of 48": "sample_offset[1]", "f1 f32 at 48 of 48": "sample_offset[4]",
             "offset near 2^31": "sample_offset[1]", "half offset 7": "sample_offset[2]", "rgb half at 44 of 48": "sample_offset[2]",
             "format 2": "sample_format[3]", "format -1": "sample_format[0]", "channels 2": "types[1].channels"}
    assert sorted(checks) == sorted(valid + list(named))
    for name in valid:
        assert checks[name] == "ok", (name, checks[name])
    for name, arg in named.items():
        assert checks[name] != "ok" and arg in checks[name], (name, checks[name])


def test_the_plan_program_is_clean_under_sanitizers(plan_lines, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own:
    no report, the same lines."""
    binary = str(tmp_path / "plan_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), PLAN_SRC, "-o", binary])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout == plan_lines[1]


def test_the_plan_is_pure():
    """statmc_records_plan.h names no HIP call and keeps no state: it includes nothing but the C headers and the ABI's."""
    src = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_records_plan.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "hip" not in code.lower() and "static" not in code and "thread_local" not in code
    assert re.findall(r"#include\s+(\S+)", code) == ["<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/statmc.h"']
