"""statmc_compact_offsets / statmc_compact_accumulate (include/statmc.h) without a GPU: the host checks of
statmc_amd/csrc/statmc_compact_args.h -- compiled into tests/cpp/test_compact_args.cpp, plain and under AddressSanitizer and UBSan --,
what the built library answers without a device, the symbols, the header's include list and the numpy restatement
(tests/compact_reference.py) that the GPU tests hold the device to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compact_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_compact_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_compact_args.h")
MIB = 1 << 20
COUNTS_AT, OFFSETS_AT, OWNERS_AT, WS_AT, ARENA_AT, STATE_AT = (i * 16 * MIB for i in range(1, 7))   # made-up images, 16 MiB apart
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
    assert int(run_args(build.COMPACT_ARGS_BIN).split()[1]) > 200      # every refusal, the clamp, the byte map above 2^31 and 2^33


def test_the_args_program_is_clean_under_sanitizers(tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same line."""
    from statmc_amd import build
    build.build_tools()
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "include")    # statmc_device.h includes the HIP runtime's header
    binary = str(tmp_path / "compact_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert run_args(binary) == run_args(build.COMPACT_ARGS_BIN)


def test_the_include_list_of_the_args_header():
    """Pure host code: the C headers its messages and integer types need, the C ABI and the accumulation family's rules."""
    includes = re.findall(r"^#include\s+(\S+)", open(ARGS_HEADER).read(), re.M)
    assert sorted(includes) == sorted(["<stdarg.h>", "<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/statmc.h"', '"statmc_accumulate_args.h"'])
    body = open(ARGS_HEADER).read()
    assert not re.search(r"\bhip[A-Z]\w*\(", body) and "thread_local" not in body and not re.search(r"^static\s+[^(]*;", body, re.M)


# ---------------------------------------------------------------- 2. the library, without a device
def test_symbols_are_exported_declared_and_wrapped(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "size_t statmc_compact_offsets_workspace": "uint16_t width, uint16_t height",
        "int statmc_compact_offsets": "uint16_t width, uint16_t height, const int32_t *sample_counts, int32_t cap, int64_t *offsets, "
                                      "int32_t *owners, int64_t owners_capacity, void *workspace, size_t workspace_bytes, void *stream",
        "int statmc_compact_accumulate": "uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats, "
                                         "int n_types, const int64_t *offsets, int64_t n_samples, int32_t split_above, void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, sym
        assert " ".join(re.sub(r"/\*.*?\*/", "", decl.group(1)).split()) == args, sym
    debug = open(os.path.join(ROOT, "include", "statmc_debug.h")).read()
    for sym in ("statmc_debug_compact_path", "statmc_debug_last_compact_path"):
        assert hasattr(lib, sym) and re.search(r"int %s\(" % sym, debug), sym
    assert (api.COMPACT_PATH_STAGED, api.COMPACT_PATH_DIRECT, api.COMPACT_PATH_SPLIT) == tuple(
        int(re.search(r"#define STATMC_COMPACT_PATH_%s (\d+)" % n, debug).group(1)) for n in ("STAGED", "DIRECT", "SPLIT"))
    assert not any(s.startswith("statmc_accumulate") for s in decls)      # the accumulate table of tests/test_accumulate_entries_cpu.py stays whole
    assert "statmc_compact.hip" in build.SOURCES and "statmc_compact_args.h" in build.HEADERS and "statmc_scan.h" in build.HEADERS
    for f in (api.compact_offsets, api.compact_accumulate, api.make_stat_type_compact, api.compact_offsets_workspace, film.FilmStats.accumulate_compact):
        assert callable(f)


def test_the_workspace_helper_needs_no_device(lib):
    from statmc_amd import api
    before = 0
    for w, h in ((1, 1), (3, 1), (37, 29), (64, 32), (64, 48), (1920, 1080), (3840, 2160), (65535, 65535)):
        b = api.compact_offsets_workspace(w, h)
        assert b == ref.workspace_bytes(w, h) and b % 8 == 0 and b >= before, (w, h)
        before = b
    assert api.compact_offsets_workspace(1920, 1080) == 2025 * 8


def stat_types(api, n, samples=ARENA_AT, channels=3):
    arr = (api.StatType * max(n, 1))()
    for i in range(n):
        t = arr[i]
        t.channels, t.transform, t.max_moment = channels, 1, 3
        t.samples = samples + i * MIB
        t.n, t.mean, t.m2, t.m3 = STATE_AT, STATE_AT + MIB, STATE_AT + 2 * MIB, STATE_AT + 3 * MIB
        t.film_mean, t.film_m2 = STATE_AT + 4 * MIB, STATE_AT + 5 * MIB
    return arr


def offsets_calls():
    """name -> (arguments, None for a valid call or the words the message must carry)"""
    ws = ref.workspace_bytes(FW, FH)
    px = FW * FH
    base = dict(width=FW, height=FH, counts=COUNTS_AT, cap=INT32_MAX, offsets=OFFSETS_AT, owners=OWNERS_AT, capacity=1000, ws=WS_AT, ws_bytes=ws)
    t = {}

    def add(name, want, **kw):
        c = dict(base)
        c.update(kw)
        t[name] = (c, want)
    add("valid", None)
    add("valid_no_owners", None, owners=0, capacity=0)
    add("valid_cap_zero", None, cap=0)
    add("valid_counts_anywhere", None, counts=COUNTS_AT + 4)
    add("valid_larger_workspace", None, ws_bytes=ws + 4096)
    add("valid_offsets_right_behind_counts", None, offsets=COUNTS_AT + px * 4)
    add("zero_width", ["width"], width=0)
    add("zero_height", ["height"], height=0)
    add("null_counts", ["null sample_counts"], counts=0)
    add("null_offsets", ["null offsets"], offsets=0)
    add("null_workspace", ["null workspace"], ws=0)
    add("misaligned_counts", ["sample_counts", "4-byte"], counts=COUNTS_AT + 2)
    add("misaligned_offsets", ["offsets", "8-byte"], offsets=OFFSETS_AT + 4)
    add("misaligned_owners", ["owners", "4-byte"], owners=OWNERS_AT + 2)
    add("misaligned_workspace", ["workspace", "8-byte"], ws=WS_AT + 4)
    add("negative_cap", ["cap"], cap=-1)
    add("negative_capacity", ["owners_capacity"], capacity=-1)
    add("capacity_without_owners", ["owners_capacity", "null owners"], owners=0)
    add("workspace_one_byte_short", ["workspace_bytes", str(ws)], ws_bytes=ws - 1)
    add("offsets_over_counts", ["offsets overlaps sample_counts"], offsets=COUNTS_AT + px * 4 - 8)
    add("offsets_over_workspace", ["offsets overlaps workspace"], ws=OFFSETS_AT + px * 8)
    add("owners_over_counts", ["owners overlaps sample_counts"], owners=COUNTS_AT + 400)
    add("owners_over_workspace", ["owners overlaps workspace"], owners=WS_AT + 16)
    add("owners_over_offsets", ["owners overlaps offsets"], owners=OFFSETS_AT - 3996)
    return t


def accumulate_calls(api):
    base = dict(width=FW, height=FH, n_types=4, types=True, formats=None, offsets=OFFSETS_AT, n_samples=1000, split_above=256, samples=ARENA_AT)
    t = {}

    def add(name, want, **kw):
        c = dict(base)
        c.update(kw)
        t[name] = (c, want)
    add("valid", None)
    add("valid_never_split", None, split_above=INT32_MAX)
    add("valid_half", None, formats=[1, 1, 1, 1], samples=ARENA_AT + 2)
    add("valid_arena_at_4", None, samples=ARENA_AT + 4)
    add("valid_above_2_31", None, n_samples=1 << 33)
    add("too_many_types", ["n_types"], n_types=17)
    add("negative_types", ["n_types"], n_types=-1)
    add("null_types", ["null types"], types=False)
    add("null_offsets", ["null offsets"], offsets=0)
    add("negative_samples", ["n_samples"], n_samples=-1)
    add("bad_format", ["sample_formats[1]"], formats=[0, 5, 0, 0])
    add("odd_half_arena", ["types[0]", "odd"], formats=[1, 0, 0, 0], samples=ARENA_AT + 1)
    add("misaligned_fp32_arena", ["types[0]", "4-byte"], samples=ARENA_AT + 2)
    add("misaligned_offsets", ["offsets", "8-byte"], offsets=OFFSETS_AT + 4)
    add("split_above_zero", ["split_above"], split_above=0)
    add("split_above_negative", ["split_above"], split_above=-7)
    return t


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every invalid call is refused with its argument named whether or not a device is set
    up; a valid call gets as far as the device check; zero types or zero samples get there too (the no-op comes behind it)."""
    import torch
    from statmc_amd import api
    no_device = not torch.cuda.is_available()
    table = offsets_calls()
    assert sum(w is not None for _, w in table.values()) >= 18
    for name, (c, want) in table.items():
        call = lambda: lib.statmc_compact_offsets(c["width"], c["height"], c["counts"] or None, c["cap"], c["offsets"] or None, c["owners"] or None,
                                                  c["capacity"], c["ws"] or None, c["ws_bytes"], None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif no_device:     # a valid call would run on made-up pointers (tests/test_compact_offsets_gpu.py runs real ones)
            assert call() == api.ERR_NO_DEVICE and b"setup" in lib.statmc_last_error(), name
    table = accumulate_calls(api)
    assert sum(w is not None for _, w in table.values()) >= 11
    for name, (c, want) in table.items():
        types = stat_types(api, max(c["n_types"], 0) if c["n_types"] <= 16 else 16, samples=c["samples"]) if c["types"] else None
        fmts = (C.c_int32 * 16)(*(c["formats"] + [0] * 12)) if c["formats"] else None
        call = lambda: lib.statmc_compact_accumulate(c["width"], c["height"], types, fmts, c["n_types"], c["offsets"] or None, c["n_samples"],
                                                     c["split_above"], None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
            assert lib.statmc_debug_last_compact_path() == 0, name       # a refused call launched nothing
        elif no_device:
            assert call() == api.ERR_NO_DEVICE and b"setup" in lib.statmc_last_error(), name
    if no_device:
        assert lib.statmc_compact_accumulate(FW, FH, None, None, 0, None, 1000, 256, None) == api.ERR_NO_DEVICE
        assert lib.statmc_compact_accumulate(FW, FH, None, None, 4, None, 0, 256, None) == api.ERR_NO_DEVICE


# ---------------------------------------------------------------- 3. the restatement's own properties
def test_the_restatement_of_the_offsets():
    counts = np.array([[3, 0, -2], [7, 1, 0]], np.int32)
    assert ref.offsets_ref(counts).tolist() == [0, 3, 3, 3, 10, 11, 11] and ref.offsets_ref(counts).dtype == np.int64
    assert ref.offsets_ref(counts, cap=2).tolist() == [0, 2, 2, 2, 4, 5, 5]
    assert ref.offsets_ref(counts, cap=0).tolist() == [0] * 7
    assert ref.owners_ref(counts, 13).tolist() == [0, 0, 0, 3, 3, 3, 3, 3, 3, 3, 4, -1, -1]
    assert ref.owners_ref(counts, 5).tolist() == [0, 0, 0, 3, 3] and ref.owners_ref(counts, 0).size == 0
    big = np.full((2, 3), INT32_MAX, np.int32)
    assert ref.offsets_ref(big)[-1] == 6 * INT32_MAX      # int64 sums: beyond 2^31 without a wrap


def test_the_restatement_of_the_run_clamp():
    start, end = ref.clamp_runs([0, 4, -3, 9, 7, 50, 12], 20)
    assert start.tolist() == [0, 4, 0, 9, 7, 20] and end.tolist() == [4, 4, 9, 9, 20, 20]
    assert np.all((0 <= start) & (start <= end) & (end <= 20))
    pixels, positions = ref.records_of_runs(start, end)
    assert pixels.tolist() == [0] * 4 + [2] * 9 + [4] * 13 and positions.tolist() == list(range(4)) + list(range(9)) + list(range(7, 20))
