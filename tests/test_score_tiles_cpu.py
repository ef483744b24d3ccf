"""statmc_score_tiles (include/statmc.h) without a GPU: the restatement (tests/score_tiles_reference.py) against a brute-force sum
in Fractions and against score_sum_reference where one tile covers the film; the argument checks, the fill and the finalisation of
statmc_amd/csrc/statmc_score_tiles_args.h -- compiled alone into tests/cpp/test_score_tiles_args.cpp, plain and under
AddressSanitizer and UBSan -- against a Python restatement of the header's rules, in the header's order, and against the restatement's
planes bit for bit; the symbol, the ctypes mirror and what the built library answers without a device."""
import ctypes as C
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import score_sum_reference as sum_ref
import score_tiles_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_score_tiles_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_score_tiles_args.h")
F32 = np.float32
FW, FH, TILE = 64, 48, 16
N_TILES = 4 * 3
MIB = 1 << 20
SCORE_AT = 16 * MIB
PLANE_AT = {p: (i + 2) * 16 * MIB for i, p in enumerate(ref.PLANES)}      # made-up planes, 16 MiB apart
ENTRY = {p: 8 if p in ("sum", "sum_sq") else 4 for p in ref.PLANES}
PX = FW * FH * 4
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


# ---------------------------------------------------------------- 1. the restatement
def brute(bits, ck):
    """one tile from its float bits, a pixel at a time, in Fractions: (sum, sum of squares, mean or None, counts, max key)"""
    total = total_sq = Fraction(0)
    counted = n_zero = n_inf = n_clip = top = 0
    for b in bits:
        b = int(b)
        k = 0 if (b & 0x7FFFFFFF) > 0x7F800000 or b >> 31 else b
        n_zero, n_inf, n_clip, top = n_zero + (k == 0), n_inf + (k == 0x7F800000), n_clip + (k > ck), max(top, k)
        c = min(k, ck)
        if c == 0x7F800000:
            continue
        e, m = c >> 23, c & 0x7FFFFF
        v = Fraction(m, 2 ** 149) if e == 0 else Fraction(m | 0x800000, 2 ** 23) * Fraction(2) ** (e - 127)
        total, total_sq, counted = total + v, total_sq + v * v, counted + 1
    return total, total_sq, (total / counted if counted else None), (len(bits), n_zero, n_inf, n_clip), top


def nearest_f32_by_neighbours(x):
    """the float32 nearest to the Fraction x >= 0, ties to even, from numpy's two neighbours of a first guess"""
    guess = F32(float(x))      # (rounded twice: only a starting point)
    best = None
    for cand in (np.nextafter(guess, F32(-np.inf)), guess, np.nextafter(guess, F32(np.inf))):
        if not np.isfinite(cand) or cand < 0:
            continue
        d = abs(Fraction(float(cand)) - x)
        even = int(np.array([cand], F32).view(np.uint32)[0]) % 2 == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, even, cand)
    return int(np.array([best[2]], F32).view(np.uint32)[0])


def test_the_restatement_equals_a_brute_force_sum_on_tiny_tiles():
    rng = np.random.default_rng(11)
    every = rng.integers(0, 2 ** 32, (11, 19), dtype=np.uint64).astype(np.uint32)
    narrow = ((rng.integers(100, 150, (11, 19)).astype(np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, (11, 19)).astype(np.uint32))
    narrow[3, 4], narrow[9, 17], narrow[0, 0] = 0x7F800000, 0, 0x80000000
    for bits in (every, narrow):
        for cap in (INF, 1.0, float(bits_f32(int(np.sort(sum_ref.keys_of(bits.view(F32)))[100]))), 0.0, -3.0):
            ck = sum_ref.key_of(cap)
            w = ref.tiles_ref(bits.view(F32), 8, cap)
            assert w["sum"].shape == (2, 3) and w["sum"].dtype == np.float64 and w["mean"].dtype == F32 and w["n_px"].dtype == np.int32
            for j in range(2):
                for i in range(3):
                    total, total_sq, mean, counts, top = brute(bits[8 * j:8 * j + 8, 8 * i:8 * i + 8].reshape(-1), ck)
                    assert (int(w["n_px"][j, i]), int(w["n_zero"][j, i]), int(w["n_infinite"][j, i]), int(w["n_clipped"][j, i])) == counts
                    assert w["sum"][j, i] == float(total) and w["sum_sq"][j, i] == float(total_sq)      # Fraction -> float rounds once, correctly
                    assert int(w["max"].view(np.uint32)[j, i]) == top
                    assert int(w["mean"].view(np.uint32)[j, i]) == (nearest_f32_by_neighbours(mean) if mean is not None else 0), (cap, j, i)
    assert w["n_px"].tolist() == [[64, 64, 24], [24, 24, 9]]


def test_the_float_rounding_of_the_restatement():
    k = ref.nearest_float32_key
    unit = ref.UNIT
    assert k(Fraction(0)) == 0 and k(unit) == 1 and k(unit / 2) == 0 and k(unit * 3 / 2) == 2 and k(unit * 5 / 2) == 2      # ties to even among subnormals
    assert k(unit / 4096) == 0 and k(unit * 3 / 4) == 1
    assert k(Fraction(1)) == 0x3F800000 and k(1 + Fraction(1, 2 ** 24)) == 0x3F800000 and k(1 + Fraction(3, 2 ** 24)) == 0x3F800002
    assert k(1 + Fraction(1, 2 ** 24) + unit) == 0x3F800001      # a double would have lost the unit: float(...) rounds to the tie first
    assert F32(float(1 + Fraction(1, 2 ** 24) + unit)).view(np.uint32) == 0x3F800000
    assert k(ref.value_of_key(0x7F7FFFFF)) == 0x7F7FFFFF and k(ref.value_of_key(0x007FFFFF) + unit / 2) == 0x00800000
    # the mean of a tile: 2^-149 over 4096 pixels is +0; a and its neighbour tie to the even one
    one = np.zeros((64, 64), np.uint32)
    one[5, 7] = 1
    w = ref.tiles_ref(one.view(F32), 64, INF)
    assert w["mean"].view(np.uint32)[0, 0] == 0 and w["sum"][0, 0] == 2.0 ** -149 and not np.signbit(w["mean"][0, 0])
    for a, even in ((0x3F800000, 0x3F800000), (0x3F800001, 0x3F800002)):
        assert ref.tiles_ref(np.array([[a, a + 1]], np.uint32).view(F32), 8, INF)["mean"].view(np.uint32)[0, 0] == even
    # +inf pixels are left out of an uncapped mean, counted at a finite cap
    s = np.array([[1.0, INF, 3.0, INF]], F32)
    assert ref.tiles_ref(s, 8, INF)["mean"][0, 0] == 2.0 and ref.tiles_ref(s, 8, 2.0)["mean"][0, 0] == 1.75 and ref.tiles_ref(s, 8, 2.0)["n_clipped"][0, 0] == 3
    assert ref.tiles_ref(np.full((2, 2), INF, F32), 8, INF)["mean"].view(np.uint32)[0, 0] == 0


def test_one_tile_over_the_film_is_score_sum():
    rng = np.random.default_rng(12)
    for W, H in ((1, 1), (7, 3), (33, 64), (64, 64)):
        score = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32).view(F32)
        for cap in (INF, 1.0, 1e-30, 0.0):
            t, s = ref.tiles_ref(score, 64, cap), sum_ref.sum_ref(score, [cap])
            assert t["sum"].shape == (1, 1)
            assert (sum_ref.double_bits(t["sum"][0, 0]), sum_ref.double_bits(t["sum_sq"][0, 0])) == (sum_ref.double_bits(s["sum"][0]), sum_ref.double_bits(s["sum_sq"][0]))
            assert (int(t["n_px"][0, 0]), int(t["n_zero"][0, 0]), int(t["n_infinite"][0, 0]), int(t["n_clipped"][0, 0])) == \
                   (s["n_px"], s["n_zero"], s["n_infinite"], s["n_clipped"][0])


# ---------------------------------------------------------------- 2. the args header, alone
def call(**kw):
    c = dict(width=FW, height=FH, score=SCORE_AT, tile=TILE, cap=f32_bits(0.05), given=1, **PLANE_AT)
    c.update(kw)
    return c


def table():
    t = {}
    t["valid"] = call()
    for tile in ref.TILES:
        t["valid_tile_%d" % tile] = call(tile=tile)
    t["valid_one_plane"] = call(**{p: 0 for p in ref.PLANES if p != "max"})
    t["valid_no_doubles"] = call(sum=0, sum_sq=0)
    t["valid_infinite_zero_and_negative_caps_0"] = call(cap=f32_bits(INF))
    t["valid_infinite_zero_and_negative_caps_1"] = call(cap=f32_bits(0.0))
    t["valid_infinite_zero_and_negative_caps_2"] = call(cap=f32_bits(-INF))
    t["valid_odd_film"] = call(width=37, height=29)
    t["valid_one_pixel"] = call(width=1, height=1, tile=64)
    t["valid_unaligned_score"] = call(score=SCORE_AT + 4)
    t["valid_largest_film"] = call(width=65535, height=65535, tile=8, score=1 << 40, **{p: (i + 2) << 40 for i, p in enumerate(ref.PLANES)})
    t["valid_plane_right_behind_score"] = call(mean=SCORE_AT + PX)
    t["valid_planes_back_to_back"] = call(sum_sq=PLANE_AT["sum"] + N_TILES * 8, n_zero=PLANE_AT["n_px"] + N_TILES * 4)
    t["valid_float_plane_4_byte_aligned"] = call(mean=PLANE_AT["mean"] + 4, n_clipped=PLANE_AT["n_clipped"] + 12)
    t["zero_width"] = call(width=0)
    t["zero_height"] = call(height=0)
    t["null_score"] = call(score=0)
    t["null_out"] = call(given=0)
    t["every_plane_null"] = call(**{p: 0 for p in ref.PLANES})
    t["misaligned_score"] = call(score=SCORE_AT + 2)
    for p in ref.PLANES:
        t["misaligned_" + p] = call(**{p: PLANE_AT[p] + ENTRY[p] // 2})
    for tile in (0, -8, 4, 12, 24, 128):
        t["tile_%s" % str(tile).replace("-", "minus_")] = call(tile=tile)
    for i, b in enumerate(NAN_BITS):
        t["nan_cap_%d" % i] = call(cap=b)
    t["plane_is_score"] = call(max=SCORE_AT)
    t["plane_in_the_last_bytes_of_score"] = call(n_px=SCORE_AT + PX - 4)
    t["plane_ends_inside_score"] = call(sum=SCORE_AT - N_TILES * 8 + 8)
    t["two_planes_are_one"] = call(mean=PLANE_AT["max"])
    t["plane_ends_inside_another"] = call(sum_sq=PLANE_AT["sum"] + N_TILES * 8 - 8)
    t["plane_starts_inside_another"] = call(n_clipped=PLANE_AT["mean"] + N_TILES * 4 - 4)
    # the order of the checks: each call breaks two rules, the earlier one is named
    t["order_size_before_null"] = call(width=0, score=0)
    t["order_null_score_before_null_out"] = call(score=0, given=0)
    t["order_null_before_every_plane_null"] = call(score=0, **{p: 0 for p in ref.PLANES})
    t["order_every_plane_null_before_alignment"] = call(score=SCORE_AT + 2, **{p: 0 for p in ref.PLANES})
    t["order_score_alignment_before_plane_alignment"] = call(score=SCORE_AT + 2, sum=PLANE_AT["sum"] + 4)
    t["order_plane_alignment_before_tile"] = call(n_zero=PLANE_AT["n_zero"] + 2, tile=5)
    t["order_planes_in_the_structs_order"] = call(mean=PLANE_AT["mean"] + 1, sum_sq=PLANE_AT["sum_sq"] + 4)
    t["order_tile_before_nan"] = call(tile=5, cap=NAN_BITS[0])
    t["order_nan_before_overlap"] = call(cap=NAN_BITS[1], max=SCORE_AT)
    t["order_score_overlap_before_plane_overlap"] = call(mean=PLANE_AT["max"], max=PLANE_AT["max"], sum=SCORE_AT)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def restated(c):
    """include/statmc.h's error list, in its order: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    if c["score"] == 0:
        return ["null score"]
    if not c["given"]:
        return ["null out"]
    if all(c[p] == 0 for p in ref.PLANES):
        return ["every plane"]
    if c["score"] % 4:
        return ["score", "aligned"]
    for p in ref.PLANES:
        if c[p] % ENTRY[p]:
            return ["out->%s " % p, "%d-byte aligned" % ENTRY[p]]
    if c["tile"] not in ref.TILES:
        return ["tile = %d" % c["tile"]]
    if (c["cap"] & 0x7FFFFFFF) > 0x7F800000:
        return ["cap", "NaN"]
    px = c["width"] * c["height"] * 4
    n = -(-c["width"] // c["tile"]) * -(-c["height"] // c["tile"])
    for i, p in enumerate(ref.PLANES):
        if overlap(c[p], n * ENTRY[p], c["score"], px):
            return ["out->%s overlaps score" % p]
        for q in ref.PLANES[:i]:
            if overlap(c[p], n * ENTRY[p], c[q], n * ENTRY[q]):
                return ["out->%s overlaps out->%s" % (p, q)]
    return None


def films():
    """whole computations for the host: (float bits [H][W], tile, cap bits)"""
    rng = np.random.default_rng(5)
    f = {}
    every = rng.integers(0, 2 ** 32, (37, 29), dtype=np.uint64).astype(np.uint32)
    for tile in ref.TILES:
        f["random_bits_%d" % tile] = (every, tile, f32_bits(INF))
    mid = int(np.sort(sum_ref.keys_of(every.view(F32)))[800])
    f["random_bits_cap_present"] = (every, 8, mid)
    f["random_bits_subnormal_cap"] = (every, 16, 0x00000123)
    f["random_bits_zero_cap"] = (every, 16, f32_bits(0.0))
    f["random_bits_negative_cap"] = (every, 32, f32_bits(-2.0))
    for name, b in (("one", 0x3F800000), ("smallest_subnormal", 1), ("largest_finite", 0x7F7FFFFF), ("third", f32_bits(1 / 3))):
        f["constant_" + name] = (np.full((70, 67), b, np.uint32), 64, f32_bits(INF))
        f["constant_%s_capped_below" % name] = (np.full((9, 9), b, np.uint32), 8, max(b - 1, 0))
    f["double_tie_even"] = (np.array([[(127 - 96) << 23, 1, 0, 0]], np.uint32), 8, f32_bits(INF))
    f["double_tie_odd"] = (np.array([[(127 - 96) << 23, 1, 1, 1]], np.uint32), 8, f32_bits(INF))
    f["float_tie_even"] = (np.array([[0x3F800000, 0x3F800001]], np.uint32), 8, f32_bits(INF))
    f["float_tie_odd"] = (np.array([[0x3F800001, 0x3F800002]], np.uint32), 8, f32_bits(INF))
    one = np.zeros((64, 64), np.uint32)
    one[63, 63] = 1
    f["one_unit_over_4096_pixels"] = (one, 64, f32_bits(INF))
    f["extremes"] = (np.array([[1, 0x7F7FFFFF], [0x7F7FFFFF, 1]], np.uint32), 16, f32_bits(INF))
    f["all_infinite"] = (np.full((3, 5), 0x7F800000, np.uint32), 8, f32_bits(INF))
    f["all_infinite_capped"] = (np.full((3, 5), 0x7F800000, np.uint32), 8, 0x7F7FFFFF)
    f["all_dead"] = (np.array([[0, 0x80000000, 0xFFC00000]], np.uint32), 8, f32_bits(INF))
    return f


def write_table(path, calls, whole):
    with open(path, "w") as f:
        for name, c in calls.items():
            f.write("tiles %s %d %d %d %d %d %d %s\n" % (name, c["width"], c["height"], c["score"], c["tile"], c["cap"], c["given"],
                                                        " ".join(str(c[p]) for p in ref.PLANES)))
        for name, (bits, tile, cap) in whole.items():
            f.write("film %s %d %d %d %d %s\n" % (name, bits.shape[1], bits.shape[0], tile, cap, " ".join(str(int(b)) for b in bits.reshape(-1))))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("score_tiles") / "table.txt")
    write_table(path, table(), films())
    return path, verdicts(build.TILES_ARGS_BIN, path)


def test_the_table_states_every_error_and_valid_calls():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid"), (name, w)
    said = set(re.sub(r"out->\w+", "out->", " ".join(w)) for w in want.values() if w)
    assert len(said) >= 10, sorted(said)
    assert want["order_size_before_null"] == ["width", "height"] and want["order_null_score_before_null_out"] == ["null score"]
    assert want["order_null_before_every_plane_null"] == ["null score"] and want["order_every_plane_null_before_alignment"] == ["every plane"]
    assert want["order_score_alignment_before_plane_alignment"] == ["score", "aligned"] and want["order_plane_alignment_before_tile"][0] == "out->n_zero "
    assert want["order_planes_in_the_structs_order"][0] == "out->sum_sq " and want["order_tile_before_nan"] == ["tile = 5"]
    assert want["order_nan_before_overlap"] == ["cap", "NaN"] and want["order_score_overlap_before_plane_overlap"] == ["out->sum overlaps score"]
    assert want["two_planes_are_one"] == ["out->max overlaps out->mean"] and want["plane_starts_inside_another"] == ["out->n_clipped overlaps out->mean"]


def test_the_args_program_passes_its_division_checks_and_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(list(t) + list(films()) + ["means"])
    assert re.fullmatch(r"ok \d+", got["means"]) and int(got["means"].split()[1]) >= 1000 + 5 * 40      # the long division agreed every time
    for name, c in t.items():
        want = restated(c)
        if want is not None:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])
            for other in ["score", "tile", "cap", "width"] + ["out->" + p for p in ref.PLANES]:
                if not any(other in w for w in want):      # only the argument at fault is named
                    assert not re.search(r"(?<![\w>])%s\b" % re.escape(other), got[name]), (name, other, got[name])
        else:
            tx, ty = -(-c["width"] // c["tile"]), -(-c["height"] // c["tile"])
            assert got[name] == "ok tiles %d %d %d %08x %d" % (tx, ty, tx * ty, sum_ref.key_of(bits_f32(c["cap"])), int(c["score"] % 16 == 0)), (name, got[name])
    assert got["valid_largest_film"].split()[2:5] == ["8192", "8192", str(8192 * 8192)]


def test_whole_films_on_the_host_equal_the_restatement_bit_for_bit(args_out):
    _, out = args_out
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    for name, (bits, tile, cap) in films().items():
        w = ref.tiles_ref(bits.view(F32), tile, bits_f32(cap))
        ty, tx = w["sum"].shape
        want = "film %d %d" % (tx, ty)
        for j in range(ty):
            for i in range(tx):
                want += " %d %d %d %d %016x %016x %08x %08x" % (w["n_px"][j, i], w["n_zero"][j, i], w["n_infinite"][j, i], w["n_clipped"][j, i],
                                                               sum_ref.double_bits(w["sum"][j, i]), sum_ref.double_bits(w["sum_sq"][j, i]),
                                                               int(w["mean"].view(np.uint32)[j, i]), int(w["max"].view(np.uint32)[j, i]))
        assert got[name] == want, name
    f = films()
    assert ref.tiles_ref(f["double_tie_even"][0].view(F32), 8, INF)["sum"][0, 0] == 2.0 ** -96      # the cases that round go through the header too
    assert ref.tiles_ref(f["double_tie_odd"][0].view(F32), 8, INF)["sum"][0, 0] == 2.0 ** -96 + 2.0 ** -147
    assert ref.tiles_ref(f["float_tie_odd"][0].view(F32), 8, INF)["mean"].view(np.uint32)[0, 0] == 0x3F800002
    assert ref.tiles_ref(f["one_unit_over_4096_pixels"][0].view(F32), 64, INF)["mean"].view(np.uint32)[0, 0] == 0


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "score_tiles_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


def test_the_args_header_compiles_with_nothing_but_the_c_header(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { const uint32_t one[12] = {8}; return statmc::tile_mean_bits(one, 12, 4) == 2 ? 0 : 1; }\n' % ARGS_HEADER)
    binary = str(tmp_path / "alone")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-fsyntax-only", "-x", "c++", str(src)])      # no C++ library header at all
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", binary])
    assert subprocess.run([binary]).returncode == 0
    text = re.sub(r"//.*", "", open(ARGS_HEADER).read())
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|\basm\b|__host__|__device__", text)      # no HIP call, type or kernel, no inline assembly
    for body in re.findall(r"(?s)STATMC_SUM_HD inline [^\n]*\n.*?\n}\n", text):      # the finalisation holds no floating-point value
        assert not re.search(r"\b(float|double)\b", body), body
    assert len(re.findall(r"STATMC_SUM_HD inline", text)) == 2
    assert re.findall(r'#include "([^"]+)"', text) == ["statmc_score_sum_args.h"]


# ---------------------------------------------------------------- 3. the library, without a device
def test_the_symbol_is_exported_declared_and_mirrored(lib, tmp_path):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    assert hasattr(lib, "statmc_score_tiles") and "statmc_score_tiles" in api.EXPORTS
    decl = re.search(r"int statmc_score_tiles\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, const float *score, int tile, float cap, "
                                                       "const statmc_tile_scores *out, void *stream")
    assert re.search(r"#define STATMC_SCORE_TILES_MAX_TILE 64\b", header) and api.SCORE_TILES_MAX_TILE == max(ref.TILES) == 64
    names = [f for f, _ in api.TileScores._fields_]
    assert tuple(names) == api.TILE_PLANES == ref.PLANES
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "statmc.h"\nint main(void) {\n  printf("%zu", sizeof(statmc_tile_scores));\n'
                   + "".join('  printf(" %%zu", offsetof(statmc_tile_scores, %s));\n' % f for f in names) + "  return 0;\n}\n")
    binary = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", binary])
    got = [int(x) for x in subprocess.check_output([binary]).split()]
    ts = api.TileScores
    assert got == [C.sizeof(ts)] + [getattr(ts, f).offset for f in names] == [64] + [8 * i for i in range(8)]
    assert "statmc_score_tiles.hip" in build.SOURCES and "statmc_score_tiles_args.h" in build.HEADERS
    assert all(callable(f) for f in (api.score_tiles, api.read_tile_scores, api.tile_grid, film.FilmStats.score_tiles))
    assert api.tile_grid(70, 257, 64) == (2, 5) and api.tile_grid(1, 1, 8) == (1, 1)
    kernel = re.sub(r"//.*", "", open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_score_tiles.hip")).read())
    assert not re.search(r"\basm\b|hipMalloc|hipMemset|hipMemcpy", kernel)      # no inline assembly; nothing allocated, zeroed or copied


def test_without_a_device_the_entry_checks_its_arguments_first(lib):
    """Made-up image pointers, never dereferenced; out is a real host struct.  Every invalid call of the table is refused with its
    argument named whether or not a device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        out = api.TileScores(**{p: c[p] or None for p in ref.PLANES})
        cap = C.c_float()
        C.memmove(C.byref(cap), C.byref(C.c_uint32(c["cap"])), 4)      # the bits as they are, NaN payloads too
        run = lambda: lib.statmc_score_tiles(c["width"], c["height"], c["score"] or None, c["tile"], cap, C.byref(out) if c["given"] else None, None)
        if want is not None:
            assert run() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_score_tiles_gpu.py runs real ones)
            assert run() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()
