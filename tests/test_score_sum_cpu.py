"""statmc_score_sum (include/statmc.h) without a GPU: the restatement (tests/score_sum_reference.py) against hand-computed cases; the
argument checks, the fill and the finalisation of statmc_amd/csrc/statmc_score_sum_args.h -- compiled alone into
tests/cpp/test_score_sum_args.cpp, plain and under AddressSanitizer and UBSan -- against a Python restatement of the header's rules,
in the header's order, and against the restatement's sums bit for bit; the symbols, the ctypes mirror, the workspace helper and what
the built library answers without a device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import score_sum_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_score_sum_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_score_sum_args.h")
F32 = np.float32
FW, FH = 64, 48
MIB = 1 << 20
SCORE_AT, RESULT_AT, WS_AT = (i * 16 * MIB for i in range(1, 4))   # made-up images, 16 MiB apart
PX = FW * FH * 4
WS_BYTES = 160 * 8      # 2 class counts, 5 interval counts, 5 x 10 sum limbs, 5 x 19 square limbs: 153 64-bit words, rounded up to 8 words
RESULT_BYTES = 152
CHUNK, MAX_GRID = 1024, 768
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
INF = float("inf")


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits_f32(b):
    return np.array([b], np.uint32).view(F32)[0]


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- 1. the restatement against hand-computed cases
def test_one_pixel_per_class():
    # key 0: +0, -0, a negative, -inf, NaN of both signs; finite: a subnormal, 1.5; infinite: +inf
    s = np.array([0x00000000, 0x80000000, f32_bits(-2.0), 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000003, f32_bits(1.5), 0x7F800000], np.uint32).view(F32)
    r = ref.sum_ref(s, [INF, 1.0, 0.0, -1.0])
    assert (r["n_px"], r["n_zero"], r["n_finite"], r["n_infinite"]) == (9, 6, 2, 1)
    assert r["cap_bits"] == [0x7F800000, 0x3F800000, 0, 0] and r["n_clipped"] == [0, 2, 3, 3]
    assert r["sum"][0] == 1.5 + 3 * 2.0 ** -149 and r["sum_sq"][0] == 2.25      # +inf is left out; 9 * 2^-298 vanishes beside 2.25
    assert r["sum"][1] == 2.0 + 3 * 2.0 ** -149 and r["sum_sq"][1] == 2.0      # 1.5 and +inf both count as 1
    assert r["sum"][2:] == [0.0, 0.0] and r["sum_sq"][2:] == [0.0, 0.0]
    assert ref.means(r)[0] == ((1.5 + 3 * 2.0 ** -149) / 8, float(np.sqrt(2.25 / 8))) and ref.means(r)[1][0] == (2.0 + 3 * 2.0 ** -149) / 9


def test_units_of_the_special_keys():
    assert ref.units_of(1) == 1 and ref.units_of(0x007FFFFF) == 0x7FFFFF and ref.units_of(0x00800000) == 0x800000      # subnormals and the first normal share s = 0
    assert ref.units_of(0x01000000) == 0x800000 << 1 and ref.units_of(0x3F800000) == 1 << 149
    assert ref.units_of(0x7F7FFFFF) == 0xFFFFFF << 253 < 2 ** 277 and ref.units_of(0) == 0
    assert ref.key_of(-0.0) == ref.key_of(np.nan) == ref.key_of(-np.inf) == ref.key_of(-3.0) == 0 and ref.key_of(np.inf) == 0x7F800000


def test_two_subnormals_sum_to_a_normal():
    s = np.array([0x00400000, 0x00400000], np.uint32).view(F32)      # 2^-127 each
    r = ref.sum_ref(s, [INF])
    assert r["sum"][0] == 2.0 ** -126 and ref.double_bits(r["sum"][0]) == (1023 - 126) << 52
    assert r["sum_sq"][0] == 2.0 ** -253
    one = ref.sum_ref(np.array([1], np.uint32).view(F32), [INF])
    assert one["sum"][0] == 2.0 ** -149 and one["sum_sq"][0] == 2.0 ** -298 and ref.double_bits(one["sum_sq"][0]) == (1023 - 298) << 52


def test_a_sum_that_rounds_in_a_double():
    # 2^24 + 1 pixels of 1.0 are exact in a double: no rounding.  2^30 and one unit: 2^54 + 1 units of 2^-24 lies between the doubles
    # 2^54 and 2^54 + 4 and rounds down; with three such units 2^54 + 3 rounds up to 2^54 + 4; with two it is a tie and goes to even.
    big, unit = F32(2.0 ** 30), F32(2.0 ** -24)
    assert ref.sum_ref(np.array([1.0] * 5 + [2.0 ** -24], F32), [INF])["sum"][0] == 5 + 2.0 ** -24      # exact
    for k, want in ((1, 2.0 ** 30), (2, 2.0 ** 30), (3, 2.0 ** 30 + 4 * 2.0 ** -24), (6, 2.0 ** 30 + 8 * 2.0 ** -24)):
        r = ref.sum_ref(np.array([big] + [unit] * k, F32), [INF])
        assert r["sum"][0] == want, k      # 2: tie, 2^54 is even; 6: tie between + 4 and + 8, + 8 is even
    assert float(np.sum(np.array([big] + [unit] * 3, np.float64))) == 2.0 ** 30      # adding one at a time loses all three
    # capped: every pixel above the cap counts at the cap
    r = ref.sum_ref(np.array([big, big, unit], F32), [1.0, unit, INF])
    assert r["sum"][:2] == [2.0 + 2.0 ** -24, 3 * 2.0 ** -24] and r["n_clipped"][:3] == [2, 2, 0] and r["sum_sq"][0] == 2.0 + 2.0 ** -48


# ---------------------------------------------------------------- 2. the args header, alone
def call(**kw):
    c = dict(width=FW, height=FH, score=SCORE_AT, result=RESULT_AT, workspace=WS_AT, workspace_bytes=WS_BYTES, given=1,
             caps=[f32_bits(INF), f32_bits(0.05)], n=None)
    c.update(kw)
    if c["n"] is None:
        c["n"] = len(c["caps"])
    return c


def table():
    t = {}
    t["valid"] = call()
    t["valid_one_cap"] = call(caps=[f32_bits(1.0)])
    t["valid_four_unsorted_repeated"] = call(caps=[f32_bits(x) for x in (2.0, 0.5, 2.0, 1e-42)])
    t["valid_zero_negative_and_infinite_caps"] = call(caps=[f32_bits(x) for x in (0.0, -1.0, INF, -INF)])
    t["valid_odd_film"] = call(width=37, height=29)
    t["valid_one_pixel"] = call(width=1, height=1)
    t["valid_unaligned_score"] = call(score=SCORE_AT + 4)
    t["valid_larger_workspace"] = call(workspace_bytes=WS_BYTES + 4096)
    t["valid_largest_film"] = call(width=65535, height=65535, score=1 << 40, result=2 << 40, workspace=3 << 40)
    t["valid_more_chunks_than_the_grid"] = call(width=1280, height=720)
    t["valid_result_right_behind_score"] = call(result=SCORE_AT + PX)
    t["valid_result_right_behind_workspace"] = call(result=WS_AT + WS_BYTES)
    t["zero_width"] = call(width=0)
    t["zero_height"] = call(height=0)
    for p in ("score", "result", "workspace"):
        t["null_" + p] = call(**{p: 0})
    t["null_caps"] = call(given=0)
    t["misaligned_score"] = call(score=SCORE_AT + 2)
    t["misaligned_result"] = call(result=RESULT_AT + 4)
    t["misaligned_workspace"] = call(workspace=WS_AT + 4)
    t["no_caps"] = call(n=0)
    t["five_caps"] = call(caps=[f32_bits(1.0)] * 5)
    t["negative_n_caps"] = call(n=-1)
    for i, b in enumerate(NAN_BITS):
        t["nan_cap_%d" % i] = call(caps=[f32_bits(1.0), b])
    t["workspace_one_byte_short"] = call(workspace_bytes=WS_BYTES - 1)
    t["workspace_zero_bytes"] = call(workspace_bytes=0)
    t["result_is_score"] = call(result=SCORE_AT)
    t["result_in_the_last_bytes_of_score"] = call(result=SCORE_AT + PX - 8)
    t["result_ends_inside_score"] = call(result=SCORE_AT - RESULT_BYTES + 8)
    t["result_inside_workspace"] = call(result=WS_AT + 64)
    t["result_in_the_last_bytes_of_workspace"] = call(result=WS_AT + WS_BYTES - 8)
    t["workspace_over_score"] = call(workspace=SCORE_AT + PX - 8)
    # the order of the checks: each call breaks two rules, the earlier one is named
    t["order_size_before_null"] = call(width=0, score=0)
    t["order_null_before_alignment"] = call(workspace=0, score=SCORE_AT + 2)
    t["order_null_caps_before_n_caps"] = call(given=0, n=0)
    t["order_alignment_before_n_caps"] = call(result=RESULT_AT + 4, n=0)
    t["order_n_caps_before_nan"] = call(caps=[NAN_BITS[0]] * 5)
    t["order_nan_before_workspace_bytes"] = call(caps=[NAN_BITS[1]], workspace_bytes=0)
    t["order_workspace_bytes_before_overlap"] = call(workspace_bytes=8, result=SCORE_AT)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def restated(c):
    """include/statmc.h's error list, in its order: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    px = c["width"] * c["height"] * 4
    for p in ("score", "result"):
        if c[p] == 0:
            return ["null " + p]
    if not c["given"]:
        return ["null caps"]
    if c["workspace"] == 0:
        return ["null workspace"]
    for p, a in (("score", 4), ("result", 8), ("workspace", 8)):
        if c[p] % a:
            return [p, "aligned"]
    if not 1 <= c["n"] <= 4:
        return ["n_caps"]
    for i, b in enumerate(c["caps"][:c["n"]]):
        if (b & 0x7FFFFFFF) > 0x7F800000:
            return ["caps[%d]" % i, "NaN"]
    if c["workspace_bytes"] < WS_BYTES:
        return ["workspace_bytes", str(WS_BYTES)]
    if overlap(c["result"], RESULT_BYTES, c["score"], px):
        return ["result overlaps score"]
    if overlap(c["result"], RESULT_BYTES, c["workspace"], WS_BYTES):
        return ["result overlaps workspace"]
    if overlap(c["workspace"], WS_BYTES, c["score"], px):
        return ["workspace overlaps score"]
    return None


def slots():
    """whole computations for the host: (pixel bits, cap bits)"""
    rng = np.random.default_rng(5)
    s = {}
    every = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32)
    s["random_bits"] = (every, [f32_bits(x) for x in (INF, 1.0, 1e-30, 1e30)])
    s["random_bits_zero_caps"] = (every[:500], [f32_bits(0.0), f32_bits(-2.0)])
    s["random_bits_subnormal_cap"] = (every[:500], [0x00000123, 0x00700000, 0x00800000])
    s["random_bits_cap_present"] = (every[:500], [int(ref.keys_of(every[:500].view(F32)).max()), int(np.sort(ref.keys_of(every[:500].view(F32)))[250])])
    for name, b in (("one", 0x3F800000), ("smallest_subnormal", 1), ("largest_finite", 0x7F7FFFFF), ("third", f32_bits(1 / 3))):
        s["constant_" + name] = (np.full(3001, b, np.uint32), [f32_bits(INF), b, max(b - 1, 0), f32_bits(1e-3)])
    s["rounds"] = (np.array([f32_bits(2.0 ** 30)] + [f32_bits(2.0 ** -24)] * 3, np.uint32), [f32_bits(INF)])
    s["all_infinite"] = (np.full(7, 0x7F800000, np.uint32), [f32_bits(INF), 0x7F7FFFFF])
    s["all_dead"] = (np.array([0, 0x80000000, 0xFFC00000], np.uint32), [f32_bits(INF)])
    return s


def write_table(path, calls, whole):
    with open(path, "w") as f:
        for name, c in calls.items():
            f.write("sum %s %d %d %d %d %d %d %d %d %d %s\n" % (name, c["width"], c["height"], c["score"], c["result"], c["workspace"],
                                                              c["workspace_bytes"], c["given"], c["n"], len(c["caps"]), " ".join(str(b) for b in c["caps"])))
        for name, (px, caps) in whole.items():
            f.write("slot %s %d %s %d %s\n" % (name, len(px), " ".join(str(int(b)) for b in px), len(caps), " ".join(str(b) for b in caps)))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("score_sum") / "table.txt")
    write_table(path, table(), slots())
    return path, verdicts(build.SUM_ARGS_BIN, path)


def test_the_table_states_every_error_and_valid_calls():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid"), (name, w)
    said = set(" ".join(re.sub(r"\[\d+\]", "", x) for x in w) for w in want.values() if w)
    assert len(said) >= 13, sorted(said)
    assert want["order_size_before_null"] == ["width", "height"] and want["order_null_before_alignment"] == ["null workspace"]
    assert want["order_null_caps_before_n_caps"] == ["null caps"] and want["order_alignment_before_n_caps"] == ["result", "aligned"]
    assert want["order_n_caps_before_nan"] == ["n_caps"] and want["order_nan_before_workspace_bytes"] == ["caps[0]", "NaN"]
    assert want["order_workspace_bytes_before_overlap"][0] == "workspace_bytes"


def test_the_args_program_passes_its_finalisation_checks_and_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(list(t) + list(slots()) + ["finalisation"])
    assert re.fullmatch(r"ok \d+", got["finalisation"]) and int(got["finalisation"].split()[1]) >= 1000 + 12      # the long division agreed every time
    for name, c in t.items():
        want = restated(c)
        if want is not None:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])
            for other in ("score", "result", "workspace", "caps", "n_caps", "width"):
                if not any(other in w for w in want):      # only the argument at fault is named
                    assert not re.search(r"\b%s\b" % other, got[name].replace("statmc_score_sum_workspace", "")), (name, other, got[name])
        else:
            chunks = -(-c["width"] * c["height"] // CHUNK)
            keys = [ref.key_of(bits_f32(b)) for b in c["caps"]]
            under = [sum(1 for x in keys if x <= k) for k in keys]
            assert got[name] == "ok sum %d %d %d %d %s / %s / %s" % (WS_BYTES, chunks, min(chunks, MAX_GRID), int(c["score"] % 16 == 0),
                                                                    " ".join("%08x" % k for k in keys), " ".join("%08x" % k for k in sorted(keys)),
                                                                    " ".join(str(u) for u in under)), (name, got[name])
    assert got["valid_more_chunks_than_the_grid"].split()[3:5] == ["900", "768"]


def test_the_whole_computation_on_the_host_equals_the_restatement_bit_for_bit(args_out):
    _, out = args_out
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    for name, (px, caps) in slots().items():
        r = ref.sum_ref(px.view(F32), [bits_f32(b) for b in caps])
        want = "slot %d %d %d" % (r["n_zero"], r["n_finite"], r["n_infinite"])
        for j in range(len(caps)):
            want += " %d %016x %016x" % (r["n_clipped"][j], ref.double_bits(r["sum"][j]), ref.double_bits(r["sum_sq"][j]))
        assert got[name] == want, name
    r = ref.sum_ref(slots()["rounds"][0].view(F32), [INF])
    assert r["sum"][0] == 2.0 ** 30 + 4 * 2.0 ** -24      # the case that rounds goes through the header too


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "score_sum_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


def test_the_args_header_compiles_with_nothing_but_the_c_header(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return statmc::sum_workspace_bytes() %% 8 == 0 ? 0 : 1; }\n' % ARGS_HEADER)
    binary = str(tmp_path / "alone")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-fsyntax-only", "-x", "c++", str(src)])      # no C++ library header at all
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", binary])
    assert subprocess.run([binary]).returncode == 0
    text = re.sub(r"//.*", "", open(ARGS_HEADER).read())
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|\basm\b", text)      # no HIP call, type or kernel, no inline assembly
    assert re.findall(r"__(?:host|device)__", text) == ["__host__", "__device__"]      # once, in the macro a host compiler never sees
    assert re.findall(r'#include "([^"]+)"', text) == ["statmc_select_args.h"]


# ---------------------------------------------------------------- 3. the library, without a device
def test_symbols_are_exported_declared_and_mirrored(lib, tmp_path):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "size_t statmc_score_sum_workspace": "void",
        "int statmc_score_sum": "uint16_t width, uint16_t height, const float *score, const float *caps, int n_caps, "
                                "statmc_sum_result *result, void *workspace, size_t workspace_bytes, void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl and " ".join(decl.group(1).split()) == args, sym
    assert re.search(r"#define STATMC_SUM_MAX_CAPS 4\b", header) and api.SUM_MAX_CAPS == ref.MAX_CAPS == 4
    names = [f for f, _ in api.SumResult._fields_]
    assert names == ["n_px", "n_zero", "n_finite", "n_infinite", "n_caps", "pad", "cap_bits", "n_clipped", "sum", "sum_sq"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "statmc.h"\nint main(void) {\n  printf("%zu", sizeof(statmc_sum_result));\n'
                   + "".join('  printf(" %%zu", offsetof(statmc_sum_result, %s));\n' % f for f in names) + "  return 0;\n}\n")
    binary = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", binary])
    got = [int(x) for x in subprocess.check_output([binary]).split()]
    sr = api.SumResult
    assert got == [C.sizeof(sr)] + [getattr(sr, f).offset for f in names] == [RESULT_BYTES, 0, 8, 16, 24, 32, 36, 40, 56, 88, 120]
    assert "statmc_score_sum.hip" in build.SOURCES and "statmc_score_sum_args.h" in build.HEADERS
    assert all(callable(f) for f in (api.score_sum_workspace, api.score_sum, api.read_sum_result, film.FilmStats.score_mean))


def test_the_workspace_helper_needs_no_device(lib):
    from statmc_amd import api
    assert api.score_sum_workspace() == api.score_sum_workspace() == WS_BYTES and WS_BYTES % 8 == 0


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up image pointers, never dereferenced; caps is a real host array.  Every invalid call of the table is refused with its
    argument named whether or not a device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        arr = (C.c_float * max(len(c["caps"]), 1))()
        C.memmove(arr, (C.c_uint32 * len(c["caps"]))(*c["caps"]), 4 * len(c["caps"]))      # the bits as they are, NaN payloads too
        run = lambda: lib.statmc_score_sum(c["width"], c["height"], c["score"] or None, arr if c["given"] else None, c["n"],
                                           C.cast(c["result"], C.POINTER(api.SumResult)), c["workspace"] or None, c["workspace_bytes"], None)
        if want is not None:
            assert run() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_score_sum_gpu.py runs real ones)
            assert run() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()
