"""statmc_score_window (include/statmc.h) without a GPU: the properties of the numpy restatement (tests/score_window_reference.py)
that tests/test_score_window_gpu.py holds the device to -- the brute-force and the separable form agree, windows compose, MAX is a
max-pooling, the keys are monotone in the radius; the argument checks of statmc_amd/csrc/statmc_score_window_args.h -- compiled
alone into tests/cpp/test_score_window_args.cpp, plain and under AddressSanitizer and UBSan -- against a Python restatement of the
header's rules, in the header's order; the symbol, its declaration and its mirrors; and what the built library answers without a
device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import score_window_reference as ref
import select_reference as sel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_score_window_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_score_window_args.h")
F32 = np.float32
FILMS = [(1, 1), (67, 1), (1, 67), (5, 3), (64, 64), (65, 63), (130, 70), (257, 131)]
RADII = [0, 1, 2, 7, 20, 32]
OPS = [ref.MAX, ref.MIN]
PAIRS = [(1, 2), (7, 13), (20, 12), (3, 0)]
FW, FH = 64, 48
MIB = 1 << 20
SCORE_AT, OUT_AT = 16 * MIB, 32 * MIB      # made-up images
PX = FW * FH * 4
TILE = 32


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- 1. the restatement's own properties
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_brute_force_equals_the_separable_form_bit_for_bit(film):
    w, h = film
    for name in ("mixed_classes", "ramp"):
        s = ref.image(name, w, h)
        for op in OPS:
            for r in RADII:
                assert np.array_equal(ref.bits(ref.window_brute(s, op, r)), ref.bits(ref.window_ref(s, op, r))), (name, op, r)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_windows_compose_clipped_borders_included(film):
    w, h = film
    for name in ("lognormal", "mixed_classes"):
        s = ref.image(name, w, h)
        for op in OPS:
            for r1, r2 in PAIRS:
                twice = ref.window_ref(ref.window_ref(s, op, r1), op, r2)
                assert np.array_equal(ref.bits(twice), ref.bits(ref.window_ref(s, op, r1 + r2))), (name, op, r1, r2)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_max_is_max_pool2d_on_canonical_images(film):
    import torch
    w, h = film
    for name in ("lognormal", "mixed_classes", "ramp_mirror"):
        canon = ref.window_ref(ref.image(name, w, h), ref.MAX, 0)
        assert not np.isnan(canon).any() and not np.signbit(canon).any()
        for r in RADII:
            pooled = torch.nn.functional.max_pool2d(torch.from_numpy(canon)[None, None], kernel_size=2 * r + 1, stride=1, padding=r)[0, 0].numpy()
            assert np.array_equal(ref.bits(pooled), ref.bits(ref.window_ref(canon, ref.MAX, r))), (name, r)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_keys_are_monotone_in_the_radius(film):
    w, h = film
    s = ref.image("mixed_classes", w, h)
    for op in OPS:
        last = ref.bits(ref.window_ref(s, op, 0)).astype(np.int64)
        assert np.array_equal(last, ref.keys_image(s).astype(np.int64))      # radius 0 canonicalises
        for r in RADII[1:]:
            now = ref.bits(ref.window_ref(s, op, r)).astype(np.int64)
            assert np.all(now >= last) if op == ref.MAX else np.all(now <= last), (op, r)
            last = now


def test_the_output_is_canonical_and_radius_zero_is_the_identity_on_canonical_images():
    s = ref.image("mixed_classes", 65, 63)
    assert np.isnan(s).any() and np.signbit(s).any()
    for op in OPS:
        for r in (0, 2):
            out = ref.window_ref(s, op, r)
            assert not np.isnan(out).any() and not np.signbit(out).any()
    logn = ref.image("lognormal", 65, 63)
    for op in OPS:
        assert np.array_equal(ref.bits(ref.window_ref(logn, op, 0)), ref.bits(logn))
    assert ref.bits(ref.window_ref(np.array([[np.nan, -1.0, -0.0]], F32), ref.MIN, 0)).tolist() == [[0, 0, 0]]


def test_an_impulse_becomes_exactly_the_clipped_square():
    w, h = 21, 13
    for op in OPS:
        for site in ref.impulse_sites(w, h):
            for r in (0, 1, 7, 32):
                got = ref.window_ref(ref.impulse(w, h, site, op), op, r)
                assert np.array_equal(ref.bits(got), ref.bits(ref.impulse_answer(w, h, site, op, r))), (op, site, r)
    assert len(ref.impulse_sites(w, h)) == 9 and ref.impulse_sites(1, 1) == [(0, 0)]


# ---------------------------------------------------------------- 2. the table of calls and the restatement of include/statmc.h
def call(**kw):
    c = dict(width=FW, height=FH, score=SCORE_AT, out=OUT_AT, op=0, radius=3)
    c.update(kw)
    return c


def table():
    t = {}
    t["valid_max"] = call()
    t["valid_min"] = call(op=1)
    t["valid_radius_0"] = call(radius=0)
    t["valid_radius_32"] = call(radius=32, op=1)
    t["valid_one_pixel"] = call(width=1, height=1, radius=32)
    t["valid_odd_film"] = call(width=37, height=29)
    t["valid_one_past_a_tile"] = call(width=33, height=65)
    t["valid_largest_film"] = call(width=65535, height=65535, score=1 << 40, out=3 << 40, radius=20)
    t["valid_unaligned_score"] = call(score=SCORE_AT + 4)
    t["valid_unaligned_out"] = call(out=OUT_AT + 12)
    t["valid_out_right_behind_score"] = call(out=SCORE_AT + PX)
    t["valid_out_ends_at_score"] = call(out=SCORE_AT - PX)
    t["zero_width"] = call(width=0)
    t["zero_height"] = call(height=0)
    t["null_score"] = call(score=0)
    t["null_out"] = call(out=0)
    t["misaligned_score"] = call(score=SCORE_AT + 2)
    t["misaligned_out"] = call(out=OUT_AT + 1)
    t["op_2"] = call(op=2)
    t["op_negative"] = call(op=-1)
    t["radius_33"] = call(radius=33)
    t["radius_negative"] = call(radius=-1)
    t["out_is_score"] = call(out=SCORE_AT)
    t["out_in_the_last_bytes_of_score"] = call(out=SCORE_AT + PX - 4)
    t["out_ends_inside_score"] = call(out=SCORE_AT - PX + 4)
    # the order of the checks: each call breaks two rules, the earlier one is named
    t["order_size_before_null"] = call(width=0, score=0)
    t["order_null_before_alignment"] = call(out=0, score=SCORE_AT + 2)
    t["order_alignment_before_op"] = call(out=OUT_AT + 2, op=7)
    t["order_op_before_radius"] = call(op=2, radius=33)
    t["order_radius_before_overlap"] = call(radius=33, out=SCORE_AT)
    return t


def restated(c):
    """include/statmc.h's error list, in its order: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    for p in ("score", "out"):
        if c[p] == 0:
            return ["null " + p]
    for p in ("score", "out"):
        if c[p] % 4:
            return [p, "aligned"]
    if c["op"] not in (0, 1):
        return ["op"]
    if not 0 <= c["radius"] <= 32:
        return ["radius"]
    px = c["width"] * c["height"] * 4
    if c["out"] < c["score"] + px and c["score"] < c["out"] + px:
        return ["out overlaps score"]
    return None


def lds_bytes(radius):
    """the staged keys, (32 + 2 r)^2, and the row results, 32 rows at the odd pitch (32 + 2 r) | 1"""
    side = TILE + 2 * radius
    return (side * side + TILE * (side | 1)) * 4


def write_table(path, calls):
    with open(path, "w") as f:
        for name, c in calls.items():
            f.write("window %s %d %d %d %d %d %d\n" % (name, c["width"], c["height"], c["score"], c["out"], c["op"], c["radius"]))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("window") / "table.txt")
    write_table(path, table())
    return path, verdicts(build.WINDOW_ARGS_BIN, path)


def test_the_table_states_every_error_and_valid_calls():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid_"), (name, w)
    assert len(set(" ".join(w) for w in want.values() if w)) == 8      # size, two NULLs, two alignments, op, radius, overlap
    assert want["order_size_before_null"] == ["width", "height"] and want["order_null_before_alignment"] == ["null out"]
    assert want["order_alignment_before_op"] == ["out", "aligned"] and want["order_op_before_radius"] == ["op"]
    assert want["order_radius_before_overlap"] == ["radius"]


def test_the_args_header_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(t)
    for name, c in t.items():
        want = restated(c)
        if want is not None:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])
            for other in ("score", "out", "op", "radius", "width"):
                if not any(other in w.split() for w in want):      # only the argument at fault is named
                    assert not re.search(r"\b%s\b" % other, got[name]), (name, other, got[name])
        else:
            tiles = (-(-c["width"] // TILE), -(-c["height"] // TILE))
            assert got[name] == "ok window %d %d %d %d %d %08x" % (tiles[0], tiles[1], lds_bytes(c["radius"]), c["score"] % 16 == 0, c["out"] % 16 == 0,
                                                                  0xFFFFFFFF if c["op"] else 0), (name, got[name])
    assert got["valid_largest_film"].split()[2:4] == ["2048", "2048"]
    assert lds_bytes(32) == 49280 <= 64 * 1024 and lds_bytes(0) == (32 * 32 + 32 * 33) * 4


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "window_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


def test_the_args_header_compiles_with_nothing_but_the_c_header(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return statmc::window_lds_bytes(STATMC_SCORE_WINDOW_MAX_RADIUS) %% 4 == 0 ? 0 : 1; }\n' % ARGS_HEADER)
    binary = str(tmp_path / "alone")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-fsyntax-only", "-x", "c++", str(src)])      # no C++ library header at all
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", binary])
    assert subprocess.run([binary]).returncode == 0
    text = open(ARGS_HEADER).read()
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__device__", re.sub(r"//.*", "", text))      # no HIP call, type or qualifier
    # the C header, and the select's host-only header for the key, which is not restated here
    assert re.findall(r'#include "([^"]+)"', text) == ["../../include/statmc.h", "statmc_select_args.h"]
    kernel = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_score_window.hip")).read()
    assert "select_key(" in kernel and "0x7F800000" not in kernel      # the key is the select's, used, not restated


# ---------------------------------------------------------------- 3. the library, without a device
def test_the_symbol_is_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    assert hasattr(lib, "statmc_score_window") and "statmc_score_window" in api.EXPORTS
    decl = re.search(r"int statmc_score_window\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, const float *score, int op, int radius, "
                                                        "float *out, void *stream")
    for name, value in (("STATMC_SCORE_WINDOW_MAX", 0), ("STATMC_SCORE_WINDOW_MIN", 1), ("STATMC_SCORE_WINDOW_MAX_RADIUS", 32)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (api.SCORE_WINDOW_MAX, api.SCORE_WINDOW_MIN, api.SCORE_WINDOW_MAX_RADIUS) == (ref.MAX, ref.MIN, ref.MAX_RADIUS) == (0, 1, 32)
    assert "statmc_score_window.hip" in build.SOURCES and "statmc_score_window_args.h" in build.HEADERS
    assert list(inspect.signature(api.score_window).parameters) == ["score", "radius", "op", "out", "stream"]
    assert inspect.signature(api.score_window).parameters["op"].default == "max"
    for f in (film.FilmStats.plan_samples, film.FilmStats.score_quantiles, film.FilmStats.score_count_above):
        assert inspect.signature(f).parameters["dilate"].default == 0, f
    hpp = open(os.path.join(ROOT, "include", "statmc_denoiser.hpp")).read()
    assert len(re.findall(r"int scoreDilate = 0\)", hpp)) == 3
    assert re.search(r"void ScoreWindow\(const float \*d_in, int op, int radius, float \*d_out\)", hpp)


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up image pointers, never dereferenced.  Every invalid call of the table is refused with its argument named whether or not
    a device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        run = lambda: lib.statmc_score_window(c["width"], c["height"], c["score"] or None, c["op"], c["radius"], c["out"] or None, None)
        if want is not None:
            assert run() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_score_window_gpu.py runs real ones)
            assert run() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()


def test_the_keys_are_the_selects():
    s = ref.image("mixed_classes", 65, 63)
    assert np.array_equal(ref.keys_image(s).reshape(-1), sel.keys_of(s))
    live, sat = sel.class_counts(sel.keys_of(s))
    assert 0 < live < s.size and sat > 0 and np.isnan(s).any()
