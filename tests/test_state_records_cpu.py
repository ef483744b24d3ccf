"""statmc_state_dwords / statmc_gather_states / statmc_combine_records (include/statmc.h) without a GPU: the host checks of
statmc_amd/csrc/statmc_state_records_args.h -- compiled into tests/cpp/test_state_records_args.cpp, plain and under AddressSanitizer
and UBSan --, the symbols, the record size for every kind of stat type, and what the built library answers without a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_state_records_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_state_records_args.h")
MIB = 1 << 20
PIXELS_AT, RECORDS_AT, STATE_AT = 16 * MIB, 32 * MIB, 96 * MIB     # made-up arrays, never dereferenced
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
    assert build.STATE_ARGS_BIN in build.TOOLS and build.STATE_BIN in build.TOOLS
    build.build_tools()
    assert int(run_args(build.STATE_ARGS_BIN).split()[1]) > 150      # the record sizes, every refusal, the argument block


def test_the_args_program_is_clean_under_sanitizers(tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same line."""
    from statmc_amd import build
    build.build_tools()
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "include")    # statmc_device.h includes the HIP runtime's header
    binary = str(tmp_path / "state_records_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert run_args(binary) == run_args(build.STATE_ARGS_BIN)


def test_the_args_header_is_pure_host_code():
    body = open(ARGS_HEADER).read()
    includes = re.findall(r"^#include\s+(\S+)", body, re.M)
    assert sorted(includes) == sorted(["<stdarg.h>", "<stddef.h>", "<stdint.h>", "<stdio.h>", '"../../include/statmc.h"', '"statmc_accumulate_args.h"',
                                       '"statmc_records_plan.h"'])
    assert not re.search(r"\bhip[A-Z]\w*\(", body) and "thread_local" not in body and not re.search(r"^static\s+[^(]*;", body, re.M)


# ---------------------------------------------------------------- 2. the symbols
def test_symbols_are_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "size_t statmc_state_dwords": "int channels, int max_moment, int transform",
        "int statmc_gather_states": "uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const int32_t *pixels, "
                                    "int64_t n_records, void *const *states, void *stream",
        "int statmc_combine_records": "uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, const int32_t *pixels, "
                                      "int64_t n_records, const void *const *states, int32_t split_above, void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, sym
        assert " ".join(re.sub(r"/\*.*?\*/", "", decl.group(1)).split()) == args, sym
    assert not any(s.split()[-1].startswith("statmc_accumulate") for s in decls)      # the accumulate table of tests/test_accumulate_entries_cpu.py stays whole
    assert "statmc_state_records.hip" in build.SOURCES and "statmc_state_records_args.h" in build.HEADERS
    for f in (api.state_dwords, api.gather_states, api.combine_records, film.FilmStats.gather_states, film.FilmStats.combine_records):
        assert callable(f)
    # the producer half in the device header, on the one field list; the C++ host layer; the example kernel
    device = open(os.path.join(ROOT, "include", "statmc_device_api.hpp")).read()
    for name in ("write_record", "read_record"):
        body = re.search(r"void %s\((?:const )?int32_t \*rec\)(?: const)? \{(.*?)\n    \}" % name, device, re.S)
        assert body and "map_state(" in body.group(1), name
    host = open(os.path.join(ROOT, "include", "statmc_denoiser.hpp")).read()
    assert "void GatherStates(" in host and "void CombineRecords(" in host and "statmc_gather_states(" in host and "statmc_combine_records(" in host
    example = open(os.path.join(ROOT, "tools", "device_accumulate_example.hip")).read()
    assert "int fold_arena_records(" in example and "write_record(" in example


KINDS = [(c, t, m) for c in (3, 1) for t in (1, 0) for m in (3, 2, 1)]


def test_state_dwords_is_the_formula_for_the_twelve_kinds_and_zero_otherwise(lib):
    """No device needed.  It agrees with the device header's state_dwords<C, MAXM, TRANSFORM>(), whose body is this formula."""
    from statmc_amd import api
    assert len(KINDS) == 12
    for c, t, m in KINDS:
        assert api.state_dwords(c, m, t) == 1 + c * (m + (2 if t else 0)), (c, t, m)
    assert (api.state_dwords(3, 3, True), api.state_dwords(3, 1, False), api.state_dwords(1, 1, False)) == (16, 4, 2)
    assert lib.statmc_state_dwords(3, 3, 7) == 16                  # transform: zero or not
    for c in range(-2, 6):
        for m in range(-2, 6):
            if (c, m) not in [(k[0], k[2]) for k in KINDS]:
                assert lib.statmc_state_dwords(c, m, 0) == 0 and lib.statmc_state_dwords(c, m, 1) == 0, (c, m)
    device = open(os.path.join(ROOT, "include", "statmc_device_api.hpp")).read()
    assert re.search(r"constexpr int state_dwords\(\) \{\s*return 1 \+ C \* \(MAXM \+ \(TRANSFORM \? 2 : 0\)\);", device)


# ---------------------------------------------------------------- 3. the library, without a device
def stat_types(api, count, over):
    arr = (api.StatType * max(count, 1))()
    for i in range(count):
        t = arr[i]
        c, tr, m = KINDS[i % len(KINDS)]
        t.channels, t.transform, t.max_moment = c, tr, m
        t.n, t.mean, t.m2, t.m3 = STATE_AT, STATE_AT + MIB, STATE_AT + 2 * MIB, STATE_AT + 3 * MIB
        t.film_mean, t.film_m2 = STATE_AT + 4 * MIB, STATE_AT + 5 * MIB
    for k, (i, v) in over.items():
        setattr(arr[i], k, v)
    return arr


def calls():
    """name -> (arguments, None for a valid call or the words the message must carry, which entries: "gc", "g" or "c")"""
    base = dict(width=FW, height=FH, n_types=4, types=True, pixels=PIXELS_AT, n_records=1000, states=[RECORDS_AT + i * MIB for i in range(16)],
                split_above=256, over={})
    t = {}

    def add(name, want, who="gc", **kw):
        c = dict(base)
        c.update(kw)
        t[name] = (c, want, who)
    add("valid", None)
    add("valid_sixteen_types", None, n_types=16)
    add("valid_never_split", None, split_above=INT32_MAX)
    add("valid_split_above_one", None, split_above=1)
    add("valid_pixels_anywhere", None, pixels=PIXELS_AT + 4)
    add("valid_most_records", None, n_records=INT32_MAX)
    add("too_many_types", ["n_types"], n_types=17)
    add("negative_types", ["n_types"], n_types=-1)
    add("negative_records", ["n_records"], n_records=-1)
    add("too_many_records", ["n_records"], n_records=1 << 31)
    add("split_above_zero", ["split_above"], who="c", split_above=0)
    add("split_above_negative", ["split_above"], who="c", split_above=-7)
    add("split_above_zero_without_records", ["split_above"], who="c", split_above=0, n_records=0)
    add("null_types", ["null types"], types=False)
    add("null_pixels", ["null pixels"], pixels=0)
    add("null_states", ["null states"], states=None)
    add("misaligned_pixels", ["pixels", "4-byte"], pixels=PIXELS_AT + 2)
    add("null_record_array", ["states[1]", "null"], states=[RECORDS_AT, 0, RECORDS_AT, RECORDS_AT])
    add("misaligned_record_array", ["states[2]", "4-byte"], states=[RECORDS_AT, RECORDS_AT, RECORDS_AT + 2, RECORDS_AT])
    add("zero_width", ["width"], width=0)
    add("zero_height", ["height"], height=0)
    add("two_channels", ["types[1]", "channels"], over=dict(channels=(1, 2)))
    add("fourth_moment", ["types[0]", "max_moment"], over=dict(max_moment=(0, 4)))
    add("null_counts", ["types[2]", "null"], over=dict(n=(2, None)))
    add("null_mean", ["types[3]", "null"], over=dict(mean=(3, None)))
    add("null_m3", ["types[0]", "m3"], over=dict(m3=(0, None)))
    add("null_film_mean", ["types[0]", "film_mean"], over=dict(film_mean=(0, None)))
    add("epilogue_half_given", ["types[0]", "come together"], who="c", over=dict(mean_corr=(0, STATE_AT + 6 * MIB)))
    add("epilogue_without_third_moment", ["types[1]", "max_moment 3"], who="c",
        over=dict(mean_corr=(1, STATE_AT + 6 * MIB), discriminator=(1, STATE_AT + 7 * MIB)))
    add("valid_gather_ignores_the_epilogue", None, who="g", over=dict(mean_corr=(1, STATE_AT + 6 * MIB)))
    return t


def invoke(lib, api, c, entry):
    n_arr = min(max(c["n_types"], 0), 16)
    types = stat_types(api, n_arr, c["over"]) if c["types"] else None
    ptrs = (C.c_void_p * 16)(*[s or None for s in (c["states"] + [RECORDS_AT] * 16)[:16]]) if c["states"] is not None else None
    if entry == "g":
        return lib.statmc_gather_states(c["width"], c["height"], types, c["n_types"], c["pixels"] or None, c["n_records"], ptrs, None)
    return lib.statmc_combine_records(c["width"], c["height"], types, c["n_types"], c["pixels"] or None, c["n_records"], ptrs, c["split_above"], None)


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every malformed call is refused with its argument named whether or not a device is set
    up; a valid call gets as far as the device check; zero types or zero records is a no-op that returns OK."""
    import torch
    from statmc_amd import api
    no_device = not torch.cuda.is_available()
    table = calls()
    assert sum(w is not None for _, w, _ in table.values()) >= 22
    for name, (c, want, who) in table.items():
        for entry in who:
            rc = None if (want is None and not no_device) else invoke(lib, api, c, entry)      # a valid call would run on made-up pointers
            if want is not None:
                assert rc == api.ERR_INVALID, (name, entry)
                msg = lib.statmc_last_error().decode()
                for word in want:
                    assert word in msg, (name, entry, word, msg)
            elif no_device:
                assert rc == api.ERR_NO_DEVICE and b"setup" in lib.statmc_last_error(), (name, entry)
    # the no-ops: OK with or without a device, whatever the other arguments hold
    for entry in "gc":
        none = dict(width=FW, height=FH, n_types=0, types=False, pixels=0, n_records=1000, states=None, split_above=256, over={})
        assert invoke(lib, api, none, entry) == api.STATMC_OK, entry
        none.update(n_types=4, n_records=0, width=0)
        assert invoke(lib, api, none, entry) == api.STATMC_OK, entry
        none.update(types=True, pixels=PIXELS_AT + 2, states=[0] * 4)
        assert invoke(lib, api, none, entry) == api.STATMC_OK, entry


def test_the_python_wrappers_check_their_tensors():
    import torch
    from statmc_amd import api
    px = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError, match="pixels"):
        api.gather_states(8, 8, [], px)
    with pytest.raises(ValueError, match="pixels"):
        api.combine_records(8, 8, [], px, [])
    t = api.StatType()
    t.channels, t.transform, t.max_moment = 3, 1, 3
    with pytest.raises(ValueError, match="one state array per stat type"):
        api.combine_records(8, 8, [t], torch.zeros(5, dtype=torch.int32), [])
    with pytest.raises(ValueError, match=r"states\[0\].*5 x 16"):
        api.combine_records(8, 8, [t], torch.zeros(5, dtype=torch.int32), [torch.zeros(5, 4, dtype=torch.int32)])
