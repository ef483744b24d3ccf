"""statmc_compact_accumulate_interleaved (include/statmc.h) without a GPU: the host checks of
statmc_amd/csrc/statmc_compact_interleaved_args.h -- compiled into tests/cpp/test_compact_interleaved_args.cpp, plain and under
AddressSanitizer and UBSan as a program of its own --, what the built library answers without a device, the symbols and the header's
include list."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_compact_interleaved_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_compact_interleaved_args.h")
MIB = 1 << 20
OFFSETS_AT, RECORDS_AT, STATE_AT = 32 * MIB, 80 * MIB, 96 * MIB      # made-up images
FW, FH = 64, 48
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- 1. the args header, alone
def run_args(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert re.fullmatch(r"ok \d+ checks\n", out.stdout), out.stdout
    return out.stdout


def test_the_args_header_passes_its_program():
    from statmc_amd import build
    build.build_tools()
    assert int(run_args(build.COMPACT_ILV_ARGS_BIN).split()[1]) > 400      # every refusal in order, the clamp, the byte map, the plan


def test_the_args_program_is_clean_under_sanitizers(tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same line."""
    from statmc_amd import build
    build.build_tools()
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "include")    # statmc_device.h includes the HIP runtime's header
    binary = str(tmp_path / "compact_interleaved_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert run_args(binary) == run_args(build.COMPACT_ILV_ARGS_BIN)


def test_the_include_list_of_the_args_header():
    """Pure host code: the C headers its messages and integer types need, the C ABI, the compact entries' clamp and the records
    entries' layout rules and type sets -- pure headers both."""
    includes = re.findall(r"^#include\s+(\S+)", open(ARGS_HEADER).read(), re.M)
    assert sorted(includes) == sorted(["<stdarg.h>", "<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/statmc.h"', '"statmc_compact_args.h"',
                                       '"statmc_records_plan.h"'])
    body = open(ARGS_HEADER).read()
    assert not re.search(r"\bhip[A-Z]\w*\(", body) and "thread_local" not in body and not re.search(r"^static\s+[^(]*;", body, re.M)
    # what it reuses it does not restate
    assert "compact_run(" not in body and "records_split_chunk" not in body
    assert "check_records_interleaved(" in body and "plan_records_interleaved(" in body


def test_the_kernels_restate_none_of_the_arithmetic():
    """A lint on spelling, not evidence of reuse: the fold's section names the shared steps and no moment arithmetic of its own.
    What holds the kernels to the definition is the bitwise comparison of tests/test_compact_interleaved_gpu.py."""
    src = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_compact.hip")).read()
    fold = src[src.index("interleaved records: statmc_compact_accumulate_interleaved"):src.index("the host side")]
    for name in ("compact_run(", "compact_run_count(", "records_split_chunk(", "merge_lanes<kRecSplitLanes>", ".load(", ".add(", ".store(", "compact_record_byte("):
        assert name in fold, name
    assert "sqrt" not in fold and "powf" not in fold and "delta" not in fold      # the moments are PixelStats' business


# ---------------------------------------------------------------- 2. the library, without a device
def test_the_symbol_is_exported_declared_and_wrapped(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    head = "int statmc_compact_accumulate_interleaved"
    args = ("uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const void *records, "
            "const statmc_record_layout *layout, const int64_t *offsets, int64_t n_records, int32_t split_above, void *stream")
    sym = head.split()[-1]
    assert hasattr(lib, sym) and sym in api.EXPORTS
    decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(re.sub(r"/\*.*?\*/", "", decl.group(1)).split()) == args
    debug = open(os.path.join(ROOT, "include", "statmc_debug.h")).read()
    for s in ("statmc_debug_compact_interleaved_path", "statmc_debug_last_compact_interleaved_path", "statmc_debug_compact_interleaved_window"):
        assert hasattr(lib, s) and re.search(r"int %s\(" % s, debug), s
    names = ("FUSED_STAGED", "FUSED_DIRECT", "GENERAL", "SPLIT")
    assert tuple(getattr(api, "COMPACT_ILV_PATH_" + n) for n in names) == tuple(
        int(re.search(r"#define STATMC_COMPACT_ILV_PATH_%s (\d+)" % n, debug).group(1)) for n in names) == (1, 2, 3, 4)
    assert "statmc_compact_interleaved_args.h" in build.HEADERS and "statmc_record_field.h" in build.HEADERS
    assert build.COMPACT_ILV_ARGS_BIN in build.TOOLS and build.COMPACT_ILV_BIN in build.TOOLS
    for f in (api.compact_accumulate_interleaved, api.compact_interleaved_path, api.last_compact_interleaved_path, film.FilmStats.accumulate_compact):
        assert callable(f)
    import inspect
    assert {"records", "layout"} <= set(inspect.signature(film.FilmStats.accumulate_compact).parameters)
    hpp = open(os.path.join(ROOT, "include", "statmc_denoiser.hpp")).read()
    assert re.search(r"void AccumulateCompactInterleaved\(int64_t nRecords, const void \*d_records, const RecordLayout &layout,[^)]*"
                     r"const int64_t \*d_offsets,\s*int splitAbove = STATMC_RECORDS_SPLIT_DEFAULT\)", hpp)


def stat_types(api, kinds):
    arr = (api.StatType * max(len(kinds), 1))()
    for i, (channels, transform, max_moment) in enumerate(kinds):
        t = arr[i]
        t.channels, t.transform, t.max_moment = channels, transform, max_moment
        t.n, t.mean, t.m2, t.m3 = STATE_AT, STATE_AT + MIB, STATE_AT + 2 * MIB, STATE_AT + 3 * MIB
        t.film_mean, t.film_m2 = STATE_AT + 4 * MIB, STATE_AT + 5 * MIB
    return arr


FIVE = [(3, 1, 3), (3, 0, 1), (3, 0, 1), (1, 0, 1), (1, 0, 1)]


def calls():
    """name -> (arguments, None for a valid call or the words the message must carry)"""
    base = dict(width=FW, height=FH, kinds=FIVE, n_types=5, types=True, layout=True, records=RECORDS_AT, offsets=OFFSETS_AT, n_records=1000,
                split_above=256, stride=44, pixel_offset=0, field_offsets=[0, 12, 24, 36, 40], formats=[0, 0, 0, 0, 0])
    t = {}

    def add(name, want, **kw):
        c = dict(base)
        c.update(kw)
        t[name] = (c, want)
    add("valid", None)
    add("valid_never_split", None, split_above=INT32_MAX)
    add("valid_above_2_31", None, n_records=1 << 33)
    add("valid_padded", None, stride=48)
    add("valid_records_at_4", None, records=RECORDS_AT + 4)
    add("valid_garbage_pixel_offset", None, pixel_offset=-12345)
    add("valid_pixel_offset_behind_the_stride", None, pixel_offset=1 << 20)
    add("valid_half_features", None, stride=28, field_offsets=[0, 12, 18, 24, 26], formats=[0, 1, 1, 1, 1])
    add("too_many_types", ["n_types"], n_types=17)
    add("negative_types", ["n_types"], n_types=-1)
    add("null_types", ["null types"], types=False)
    add("null_layout", ["null layout"], layout=False)
    add("null_records", ["null records"], records=0)
    add("null_offsets", ["null offsets"], offsets=0)
    add("negative_records", ["n_records"], n_records=-1)
    add("stride_zero", ["stride"], stride=0)
    add("stride_not_a_multiple_of_4", ["stride"], stride=46)
    add("misaligned_records", ["records", "4-byte"], records=RECORDS_AT + 2)
    add("bad_format", ["sample_format[1]"], formats=[0, 5, 0, 0, 0])
    add("bad_channels", ["types[3].channels"], kinds=FIVE[:3] + [(2, 0, 1)] + FIVE[4:])
    add("negative_field_offset", ["sample_offset[0]"], field_offsets=[-4, 12, 24, 36, 40])
    add("field_behind_the_stride", ["sample_offset[2]"], field_offsets=[0, 12, 36, 36, 40])
    add("misaligned_fp32_field", ["sample_offset[1]"], field_offsets=[0, 14, 24, 36, 40])
    add("odd_half_field", ["sample_offset[4]"], formats=[0, 0, 0, 0, 1], field_offsets=[0, 12, 24, 36, 41])
    add("misaligned_offsets", ["offsets", "8-byte"], offsets=OFFSETS_AT + 4)
    add("split_above_zero", ["split_above"], split_above=0)
    add("split_above_negative", ["split_above"], split_above=-7)
    # the documented order: the earlier rule is the one named
    add("types_before_layout", ["null types"], types=False, layout=False, records=0, offsets=0)
    add("records_count_before_stride", ["n_records"], n_records=-1, stride=6, split_above=0)
    add("stride_before_fields", ["stride"], stride=6, formats=[7, 0, 0, 0, 0], offsets=OFFSETS_AT + 4)
    add("fields_before_offsets_alignment", ["sample_format[0]"], formats=[7, 0, 0, 0, 0], offsets=OFFSETS_AT + 4, split_above=0)
    add("offsets_alignment_before_split", ["offsets", "8-byte"], offsets=OFFSETS_AT + 4, split_above=0)
    return t


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every invalid call is refused with its argument named whether or not a device is set
    up; a valid call gets as far as the device check; zero types or zero records get there too (the no-op comes behind it)."""
    import torch
    from statmc_amd import api
    no_device = not torch.cuda.is_available()
    table = calls()
    assert sum(w is not None for _, w in table.values()) >= 20
    for name, (c, want) in table.items():
        types = stat_types(api, c["kinds"] + [(1, 0, 1)] * 12) if c["types"] else None
        layout = api.make_record_layout(c["stride"], c["pixel_offset"], c["field_offsets"], c["formats"]) if c["layout"] else None
        call = lambda: lib.statmc_compact_accumulate_interleaved(c["width"], c["height"], types, c["n_types"], c["records"] or None,
                                                                 C.byref(layout) if layout is not None else None, c["offsets"] or None,
                                                                 c["n_records"], c["split_above"], None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
            assert lib.statmc_debug_last_compact_interleaved_path() == 0, name       # a refused call launched nothing
        elif no_device:     # a valid call would run on made-up pointers (tests/test_compact_interleaved_gpu.py runs real ones)
            assert call() == api.ERR_NO_DEVICE and b"setup" in lib.statmc_last_error(), name
    if no_device:
        assert lib.statmc_compact_accumulate_interleaved(FW, FH, None, 0, None, None, None, 1000, 256, None) == api.ERR_NO_DEVICE
        assert lib.statmc_compact_accumulate_interleaved(FW, FH, None, 5, None, None, None, 0, 256, None) == api.ERR_NO_DEVICE
        assert lib.statmc_debug_compact_interleaved_path(1) == api.ERR_NO_DEVICE
