"""statmc_score_select / statmc_score_count_above (include/statmc.h) without a GPU: the symbols, their declarations and the ctypes
mirror; the argument checks of statmc_amd/csrc/statmc_select_args.h -- compiled alone into tests/cpp/test_select_args.cpp, plain and
under AddressSanitizer and UBSan -- against a Python restatement of the header's rules, in the header's order; the workspace helper
and what the built library answers without a device; and the properties of the numpy restatement (tests/select_reference.py) that
tests/test_score_select_gpu.py holds the device to."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plan_reference as plan_ref
import select_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_select_args.cpp")
F32 = np.float32
FW, FH = 64, 48
MIB = 1 << 20
SCORE_AT, RESULT_AT, WS_AT, COUNTS_AT = (i * 16 * MIB for i in range(1, 5))   # made-up images, 16 MiB apart
PX = FW * FH * 4
WS_BYTES = ((1 + 3 * 8) * 256 + 8) * 8     # pass 0's histogram, eight for each of the three later passes, the class counts: 64-bit words
RESULT_BYTES = 256
CHUNK, MAX_GRID = 1024, 768
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- the table of calls and the restatement of include/statmc.h
def select(**kw):
    c = dict(kind="select", width=FW, height=FH, score=SCORE_AT, result=RESULT_AT, workspace=WS_AT, workspace_bytes=WS_BYTES,
             given=1, ranks=[0, FW * FH - 1, FW * FH // 2], n=None)
    c.update(kw)
    if c["n"] is None:
        c["n"] = len(c["ranks"])
    return c


def count(**kw):
    c = dict(kind="count", width=FW, height=FH, score=SCORE_AT, counts=COUNTS_AT, given=1,
             thresholds=[f32_bits(0.0), f32_bits(-1.0), f32_bits(float("inf")), f32_bits(0.02)], n=None)
    c.update(kw)
    if c["n"] is None:
        c["n"] = len(c["thresholds"])
    return c


def table():
    t = {}
    last = FW * FH - 1
    t["valid_select"] = select()
    t["valid_select_one_rank"] = select(ranks=[7])
    t["valid_select_eight_unsorted_repeated"] = select(ranks=[last, 0, 5, 5, 1000, 3, last, 17])
    t["valid_select_odd_film"] = select(width=37, height=29, ranks=[37 * 29 - 1])
    t["valid_select_one_pixel"] = select(width=1, height=1, ranks=[0] * 8)
    t["valid_select_unaligned_score"] = select(score=SCORE_AT + 4)
    t["valid_select_larger_workspace"] = select(workspace_bytes=WS_BYTES + 4096)
    t["valid_select_largest_film"] = select(width=65535, height=65535, score=1 << 40, result=2 << 40, workspace=3 << 40, ranks=[65535 * 65535 - 1, 0])
    t["valid_select_more_chunks_than_the_grid"] = select(width=1280, height=720, ranks=[1280 * 720 - 1])
    t["valid_select_result_right_behind_score"] = select(result=SCORE_AT + PX)
    t["valid_select_result_right_behind_workspace"] = select(result=WS_AT + WS_BYTES)
    t["select_zero_width"] = select(width=0)
    t["select_zero_height"] = select(height=0)
    for p in ("score", "result", "workspace"):
        t["select_null_" + p] = select(**{p: 0})
    t["select_null_ranks"] = select(given=0)
    t["select_misaligned_score"] = select(score=SCORE_AT + 2)
    t["select_misaligned_result"] = select(result=RESULT_AT + 4)
    t["select_misaligned_workspace"] = select(workspace=WS_AT + 4)
    t["select_no_ranks"] = select(n=0)
    t["select_nine_ranks"] = select(ranks=list(range(9)))
    t["select_negative_n_ranks"] = select(n=-1)
    t["select_rank_at_the_film_size"] = select(ranks=[0, last + 1])
    t["select_negative_rank"] = select(ranks=[3, 2, -1])
    t["select_workspace_one_byte_short"] = select(workspace_bytes=WS_BYTES - 1)
    t["select_workspace_zero_bytes"] = select(workspace_bytes=0)
    t["select_result_is_score"] = select(result=SCORE_AT)
    t["select_result_in_the_last_bytes_of_score"] = select(result=SCORE_AT + PX - 8)
    t["select_result_ends_inside_score"] = select(result=SCORE_AT - RESULT_BYTES + 8)
    t["select_result_inside_workspace"] = select(result=WS_AT + 64)
    t["select_result_in_the_last_bytes_of_workspace"] = select(result=WS_AT + WS_BYTES - 8)
    t["select_workspace_over_score"] = select(workspace=SCORE_AT + PX - 8)
    # the order of the checks: each call breaks two rules, the earlier one is named
    t["select_order_size_before_null"] = select(width=0, score=0)
    t["select_order_null_before_alignment"] = select(workspace=0, score=SCORE_AT + 2)
    t["select_order_null_ranks_before_n_ranks"] = select(given=0, n=0)
    t["select_order_alignment_before_n_ranks"] = select(result=RESULT_AT + 4, n=0)
    t["select_order_n_ranks_before_ranks"] = select(ranks=[-1] * 9)
    t["select_order_ranks_before_workspace_bytes"] = select(ranks=[last + 1], workspace_bytes=0)
    t["select_order_workspace_bytes_before_overlap"] = select(workspace_bytes=8, result=SCORE_AT)

    t["valid_count"] = count()
    t["valid_count_one_threshold"] = count(thresholds=[f32_bits(1.0)])
    t["valid_count_eight_thresholds"] = count(thresholds=[f32_bits(x) for x in (0.0, -0.0, -1.0, float("inf"), float("-inf"), 1e-42, 2.0 ** 60, 3e38)])
    t["valid_count_unaligned_score"] = count(score=SCORE_AT + 12)
    t["valid_count_odd_film"] = count(width=37, height=29)
    t["valid_count_counts_right_behind_score"] = count(counts=SCORE_AT + PX)
    t["valid_count_counts_end_at_score"] = count(counts=SCORE_AT - 32)
    t["count_zero_width"] = count(width=0)
    t["count_zero_height"] = count(height=0)
    t["count_null_score"] = count(score=0)
    t["count_null_counts"] = count(counts=0)
    t["count_null_thresholds"] = count(given=0)
    t["count_misaligned_score"] = count(score=SCORE_AT + 1)
    t["count_misaligned_counts"] = count(counts=COUNTS_AT + 4)
    t["count_no_thresholds"] = count(n=0)
    t["count_nine_thresholds"] = count(thresholds=[f32_bits(1.0)] * 9)
    for i, b in enumerate(NAN_BITS):
        t["count_nan_threshold_%d" % i] = count(thresholds=[f32_bits(1.0), b])
    t["count_counts_is_score"] = count(counts=SCORE_AT)
    t["count_counts_in_the_last_bytes_of_score"] = count(counts=SCORE_AT + PX - 8)
    t["count_counts_end_inside_score"] = count(counts=SCORE_AT - 24)
    t["count_order_null_before_alignment"] = count(counts=0, score=SCORE_AT + 2)
    t["count_order_alignment_before_n_thresholds"] = count(counts=COUNTS_AT + 4, n=0)
    t["count_order_n_thresholds_before_nan"] = count(thresholds=[NAN_BITS[0]] * 9)
    t["count_order_nan_before_overlap"] = count(thresholds=[NAN_BITS[1]], counts=SCORE_AT)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def restated(c):
    """include/statmc.h's error list, in its order: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    px = c["width"] * c["height"] * 4
    if c["kind"] == "select":
        for p in ("score", "result"):
            if c[p] == 0:
                return ["null " + p]
        if not c["given"]:
            return ["null ranks"]
        if c["workspace"] == 0:
            return ["null workspace"]
        for p, a in (("score", 4), ("result", 8), ("workspace", 8)):
            if c[p] % a:
                return [p, "aligned"]
        if not 1 <= c["n"] <= 8:
            return ["n_ranks"]
        for i, r in enumerate(c["ranks"][:c["n"]]):
            if not 0 <= r < c["width"] * c["height"]:
                return ["ranks[%d]" % i]
        if c["workspace_bytes"] < WS_BYTES:
            return ["workspace_bytes", str(WS_BYTES)]
        if overlap(c["result"], RESULT_BYTES, c["score"], px):
            return ["result overlaps score"]
        if overlap(c["result"], RESULT_BYTES, c["workspace"], WS_BYTES):
            return ["result overlaps workspace"]
        if overlap(c["workspace"], WS_BYTES, c["score"], px):
            return ["workspace overlaps score"]
        return None
    for p in ("score", "counts"):
        if c[p] == 0:
            return ["null " + p]
    if not c["given"]:
        return ["null thresholds"]
    for p, a in (("score", 4), ("counts", 8)):
        if c[p] % a:
            return [p, "aligned"]
    if not 1 <= c["n"] <= 8:
        return ["n_thresholds"]
    for i, b in enumerate(c["thresholds"][:c["n"]]):
        if (b & 0x7FFFFFFF) > 0x7F800000:
            return ["thresholds[%d]" % i, "NaN"]
    if overlap(c["counts"], 8 * c["n"], c["score"], px):
        return ["counts overlaps score"]
    return None


KEY_BITS = {"plus_zero": 0, "minus_zero": 0x80000000, "minus_inf": 0xFF800000, "plus_inf": 0x7F800000, "nan": 0x7FC00000, "minus_nan": 0xFFC00000,
            "signalling_nan": 0x7F800001, "negative_subnormal": 0x80000001, "subnormal_1e-42": f32_bits(1e-42), "one": 0x3F800000,
            "minus_3.5": f32_bits(-3.5), "largest_finite": 0x7F7FFFFF}


def write_table(path, calls):
    with open(path, "w") as f:
        for name, c in calls.items():
            if c["kind"] == "select":
                f.write("select %s %d %d %d %d %d %d %d %d %d %s\n" % (name, c["width"], c["height"], c["score"], c["result"], c["workspace"],
                                                                     c["workspace_bytes"], c["given"], c["n"], len(c["ranks"]),
                                                                     " ".join(str(r) for r in c["ranks"])))
            else:
                f.write("count %s %d %d %d %d %d %d %d %s\n" % (name, c["width"], c["height"], c["score"], c["counts"], c["given"], c["n"],
                                                              len(c["thresholds"]), " ".join(str(b) for b in c["thresholds"])))
        for name, b in KEY_BITS.items():
            f.write("key %s %d\n" % (name, b))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("select") / "table.txt")
    write_table(path, table())
    return path, verdicts(build.SELECT_ARGS_BIN, path)


# ---------------------------------------------------------------- 1. the args header, alone
def test_the_table_states_every_error_and_valid_calls_of_both_entries():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid_"), (name, w)
    said = set(" ".join(re.sub(r"\[\d+\]", "", x) for x in w) for w in want.values() if w)
    assert len(said) >= 20, sorted(said)
    # the order: the two-fault calls name the earlier rule
    assert want["select_order_size_before_null"] == ["width", "height"] and want["select_order_null_before_alignment"] == ["null workspace"]
    assert want["select_order_null_ranks_before_n_ranks"] == ["null ranks"] and want["select_order_alignment_before_n_ranks"] == ["result", "aligned"]
    assert want["select_order_n_ranks_before_ranks"] == ["n_ranks"] and want["select_order_ranks_before_workspace_bytes"] == ["ranks[0]"]
    assert want["select_order_workspace_bytes_before_overlap"][0] == "workspace_bytes"
    assert want["count_order_n_thresholds_before_nan"] == ["n_thresholds"] and want["count_order_nan_before_overlap"] == ["thresholds[0]", "NaN"]


def test_the_args_header_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(list(t) + list(KEY_BITS))
    for name, c in t.items():
        want = restated(c)
        chunks = -(-c["width"] * c["height"] // CHUNK) if c["width"] and c["height"] else 0
        vec = int(c["score"] % 16 == 0)
        if want is not None:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])
            for other in ("score", "result", "workspace", "ranks", "counts", "thresholds", "n_ranks", "n_thresholds", "width"):
                if not any(other in w for w in want):      # only the argument at fault is named
                    assert not re.search(r"\b%s\b" % other, got[name].replace("statmc_score_select_workspace", "")), (name, other, got[name])
        elif c["kind"] == "select":
            assert got[name] == "ok select %d %d %d %d %s" % (WS_BYTES, chunks, min(chunks, MAX_GRID), vec, " ".join(str(r) for r in c["ranks"])), name
        else:
            keys = " ".join("%08x" % ref.keys_of(np.array([b], np.uint32).view(F32))[0] for b in c["thresholds"])
            assert got[name] == "ok count %d %d %d %s" % (chunks, min(chunks, MAX_GRID), vec, keys), (name, got[name])
    assert got["valid_select_more_chunks_than_the_grid"].split()[3:5] == ["900", "768"]      # the stride loop runs twice there
    for name, b in KEY_BITS.items():
        assert got[name] == "key %08x" % ref.keys_of(np.array([b], np.uint32).view(F32))[0], name
    assert got["nan"] == got["minus_nan"] == got["signalling_nan"] == got["minus_zero"] == got["minus_inf"] == got["negative_subnormal"] == "key 00000000"
    assert got["plus_inf"] == "key 7f800000" and got["subnormal_1e-42"] == "key %08x" % f32_bits(1e-42)


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "select_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


def test_the_args_header_compiles_with_nothing_but_the_c_header(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return statmc::select_workspace_bytes() %% 8 == 0 ? 0 : 1; }\n'
                   % os.path.join(ROOT, "statmc_amd", "csrc", "statmc_select_args.h"))
    binary = str(tmp_path / "alone")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-fsyntax-only", "-x", "c++", str(src)])      # no C++ library header at all
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", binary])
    assert subprocess.run([binary]).returncode == 0
    text = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_select_args.h")).read()
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__", re.sub(r"//.*", "", text))      # no HIP call, type or qualifier
    assert re.findall(r'#include "([^"]+)"', text) == ["../../include/statmc.h"]


# ---------------------------------------------------------------- 2. the library, without a device
def test_symbols_are_exported_declared_and_mirrored(lib, tmp_path):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "size_t statmc_score_select_workspace": "void",
        "int statmc_score_select": "uint16_t width, uint16_t height, const float *score, const int64_t *ranks, int n_ranks, "
                                   "statmc_select_result *result, void *workspace, size_t workspace_bytes, void *stream",
        "int statmc_score_count_above": "uint16_t width, uint16_t height, const float *score, const float *thresholds, int n_thresholds, "
                                        "int64_t *counts, void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl and " ".join(decl.group(1).split()) == args, sym
    assert re.search(r"#define STATMC_SELECT_MAX_RANKS 8\b", header) and api.SELECT_MAX_RANKS == ref.MAX_RANKS == 8
    # sizeof / offsetof by the C compiler against the ctypes mirror
    names = [f for f, _ in api.SelectResult._fields_]
    assert names == ["n_px", "n_live", "n_saturated", "n_ranks", "pad", "rank", "value_bits", "n_below", "n_equal"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "statmc.h"\nint main(void) {\n  printf("%zu", sizeof(statmc_select_result));\n'
                   + "".join('  printf(" %%zu", offsetof(statmc_select_result, %s));\n' % f for f in names) + "  return 0;\n}\n")
    binary = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", binary])
    got = [int(x) for x in subprocess.check_output([binary]).split()]
    sr = api.SelectResult
    assert got == [C.sizeof(sr)] + [getattr(sr, f).offset for f in names] == [256, 0, 8, 16, 24, 28, 32, 96, 128, 192]
    assert "statmc_select.hip" in build.SOURCES and "statmc_select_args.h" in build.HEADERS
    assert all(callable(f) for f in (api.score_select_workspace, api.score_select, api.score_count_above, api.read_select_result,
                                     film.FilmStats.score_quantiles, film.FilmStats.score_count_above))
    assert (ref.LIVE_LO, ref.LIVE_HI) == (f32_bits(float(plan_ref.LIVE_LO)), f32_bits(float(plan_ref.LIVE_HI)))      # the plan's classes, on keys


def test_the_workspace_helper_needs_no_device(lib):
    from statmc_amd import api
    assert api.score_select_workspace() == api.score_select_workspace() == WS_BYTES and WS_BYTES % 8 == 0
    assert WS_BYTES < 64 * 1024


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up image pointers, never dereferenced; ranks and thresholds are real host arrays.  Every invalid call of the table is
    refused with its argument named whether or not a device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        if c["kind"] == "select":
            arr = (C.c_int64 * max(len(c["ranks"]), 1))(*c["ranks"])
            call = lambda: lib.statmc_score_select(c["width"], c["height"], c["score"] or None, arr if c["given"] else None, c["n"],
                                                   C.cast(c["result"], C.POINTER(api.SelectResult)), c["workspace"] or None, c["workspace_bytes"], None)
        else:
            arr = (C.c_float * max(len(c["thresholds"]), 1))()
            C.memmove(arr, (C.c_uint32 * len(c["thresholds"]))(*c["thresholds"]), 4 * len(c["thresholds"]))      # the bits as they are, NaN payloads too
            call = lambda: lib.statmc_score_count_above(c["width"], c["height"], c["score"] or None, arr if c["given"] else None, c["n"],
                                                        c["counts"] or None, None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_score_select_gpu.py runs real ones)
            assert call() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- 3. the restatement's own properties
def positive_images():
    """float32 images without NaN and without the sign bit: there the key order is the value order"""
    rng = np.random.default_rng(11)
    h, w = 23, 31
    logn = plan_ref.lognormal_scores(h, w, 3)
    ties = np.round(logn * 4) / 4
    special = logn.copy().reshape(-1)
    special[::5] = 0
    special[1::7] = np.inf
    special[2::11] = F32(1e-42)
    special[3::13] = F32(3e38)
    return {"lognormal": logn, "ties": ties.astype(F32), "special": special.reshape(h, w), "constant": np.full((h, w), 0.75, F32),
            "one_pixel": np.array([[2.5]], F32), "two_values": np.where(rng.random((h, w)) < 0.3, F32(0.5), F32(2)).astype(F32)}


def some_ranks(px, rng):
    return [[0], [px - 1], [px // 2], [0, px - 1, px // 2], [int(r) for r in rng.integers(0, px, 8)], [px // 3] * 8]


def test_the_restatement_is_np_sort_on_the_values_where_nothing_is_negative_or_nan():
    rng = np.random.default_rng(4)
    for name, s in positive_images().items():
        flat = np.sort(s.reshape(-1))
        for ranks in some_ranks(s.size, rng):
            r = ref.select_ref(s, ranks)
            assert r["n_px"] == s.size and r["n_ranks"] == len(ranks) and r["rank"] == ranks
            assert np.array_equal(ref.values_of(r["value_bits"]).view(np.uint32), flat[ranks].view(np.uint32)), (name, ranks)
            for k, v in zip(ranks, ref.values_of(r["value_bits"])):
                i = ranks.index(k)
                assert r["n_below"][i] == int((s < v).sum()) and r["n_equal"][i] == int((s == v).sum()), (name, k)


def test_the_rank_lies_in_its_run_and_the_values_are_monotone_in_the_rank():
    rng = np.random.default_rng(6)
    images = dict(positive_images())
    mixed = images["lognormal"].copy().reshape(-1)
    mixed[::3] = np.nan
    mixed[1::5] = -2.0
    mixed[2::7] = -np.inf
    images["mixed"] = mixed.reshape(images["lognormal"].shape)
    for name, s in images.items():
        for ranks in some_ranks(s.size, rng):
            r = ref.select_ref(s, ranks)
            for i, k in enumerate(ranks):
                assert r["n_below"][i] <= k < r["n_below"][i] + r["n_equal"][i], (name, k)
            order = np.argsort(ranks, kind="stable")
            vals = [r["value_bits"][i] for i in order]
            assert all(a <= b for a, b in zip(vals, vals[1:])), (name, ranks)
        live, sat = plan_ref.classes(s)
        r = ref.select_ref(s, [0])
        assert (r["n_live"], r["n_saturated"]) == (int(live.sum()), int(sat.sum())), name      # the plan's classes
    r = ref.select_ref(images["mixed"], [0, images["mixed"].size - 1])
    dead_low = int(np.isnan(mixed).sum() + (mixed < 0).sum())
    assert r["value_bits"][0] == 0 and r["n_below"][0] == 0 and r["n_equal"][0] == dead_low      # NaN and negatives sort with +0


def test_keys_of_the_special_values():
    assert ref.key_of(-0.0) == 0 and ref.key_of(-np.inf) == 0 and ref.key_of(-3.5) == 0
    nans = np.array(NAN_BITS, np.uint32).view(F32)
    assert np.all(np.isnan(nans)) and np.all(ref.keys_of(nans) == 0)
    assert ref.keys_of(np.array([0x80000001], np.uint32).view(F32))[0] == 0      # a negative subnormal
    tiny = F32(1e-42)
    assert 0 < tiny < np.finfo(F32).tiny and ref.key_of(tiny) == f32_bits(1e-42) > ref.key_of(0.0) == 0      # a subnormal is its bits, above +0
    assert ref.key_of(np.inf) == 0x7F800000 and ref.key_of(1.0) == 0x3F800000
    s = np.array([[tiny, 0.0, -0.0, np.nan, 1.0]], F32)
    r = ref.select_ref(s, [0, 2, 3, 4])
    assert r["value_bits"] == [0, 0, f32_bits(1e-42), 0x3F800000] and r["n_equal"][0] == 3 and r["n_below"][2] == 3
    assert (ref.key_of(2.0 ** 60), ref.key_of(2.0 ** -60)) == (ref.LIVE_HI, ref.LIVE_LO)


def test_count_above_is_the_select_seen_from_the_other_side():
    rng = np.random.default_rng(8)
    for name, s in positive_images().items():
        ranks = [int(r) for r in rng.integers(0, s.size, 8)]
        r = ref.select_ref(s, ranks)
        above = ref.count_above_ref(s, ref.values_of(r["value_bits"]))
        assert above == [s.size - b - e for b, e in zip(r["n_below"], r["n_equal"])], name
        assert ref.count_above_ref(s, [-1.0, 0.0, -0.0, -np.inf]) == [int((s > 0).sum())] * 4      # a negative threshold counts the pixels above +0
        assert ref.count_above_ref(s, [np.inf]) == [0]


def test_nearest_rank_is_exact_in_integers():
    assert [ref.nearest_rank(q, 3072) for q in (0, 0.5, 0.95, 1)] == [0, 1535, 2918, 3071]
    assert ref.nearest_rank(0.5, 1) == 0 and ref.nearest_rank(1, 1) == 0 and ref.nearest_rank(1e-300, 10) == 0
    assert ref.nearest_rank(0.25, 4) == 0 and ref.nearest_rank(0.25, 5) == 1 and ref.nearest_rank(1, 65535 * 65535) == 65535 * 65535 - 1
    from fractions import Fraction
    assert ref.nearest_rank(Fraction(95, 100), 100) == 94 and ref.nearest_rank(0.95, 100) == 94      # the double 0.95 lies just below 95 / 100
