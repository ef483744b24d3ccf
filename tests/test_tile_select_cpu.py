"""statmc_score_tile_select and statmc_gate_tiles (include/statmc.h) without a GPU: the restatement (tests/tile_select_reference.py)
against a brute-force Python loop on tiny films and against select_reference where one tile covers the film; the argument checks, the
fills, the rank rule and the host evaluation of statmc_amd/csrc/statmc_tile_select_args.h -- compiled alone into
tests/cpp/test_tile_select_args.cpp, plain and under AddressSanitizer and UBSan -- against a Python restatement of the header's rules,
in the header's order, and against the restatement's planes bit for bit; the symbols, the ctypes mirrors and what the built library
answers without a device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import select_reference as sel_ref
import tile_select_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_tile_select_args.cpp")
ARGS_HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_tile_select_args.h")
F32 = np.float32
FW, FH, TILE = 64, 48, 16
N_TILES = 4 * 3
MIB = 1 << 20
SCORE_AT = 16 * MIB
PX = FW * FH * 4
PLANE_BYTES = N_TILES * 4
SLOTS = [(f, i) for f in ref.FIELDS for i in range(4)]      # the struct's order
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)
INF = float("inf")


def plane_at(f, i):
    return (2 + ref.FIELDS.index(f) * 4 + i) * 16 * MIB      # made-up planes, 16 MiB apart


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
def test_the_restatement_equals_a_brute_force_loop_on_tiny_films():
    rng = np.random.default_rng(21)
    every = rng.integers(0, 2 ** 32, (11, 19), dtype=np.uint64).astype(np.uint32)
    ties = rng.choice(np.array([0, 1, 0x3F800000, 0x7F800000, 0x80000000, 0x7FC00000], np.uint32), (11, 19))
    for bits in (every, ties):
        for tile in (8, 16):
            for nums, den in (([0, 10, 19, 20], 20), ([1], 2), ([65535, 65536], 65536), ([0], 1)):
                w = ref.tile_select_ref(bits.view(F32), tile, nums, den)
                b = ref.tile_select_brute(bits.view(F32), tile, nums, den)
                assert len(b) == w["value"][0].size * len(nums)
                for (j, i, r), (v, nb, ne) in b.items():
                    assert (int(w["value"][r].view(np.uint32)[j, i]), int(w["n_below"][r][j, i]), int(w["n_equal"][r][j, i])) == (v, nb, ne)
                    assert nb <= int(w["rank"][r][j, i]) < nb + ne
                assert w["value"][0].dtype == F32 and w["n_below"][0].dtype == np.int32 and w["n_equal"][0].dtype == np.int32
    assert w["value"][0].shape == (1, 2)
    assert (ties.view(np.uint32) == 0x7F800000).any() and max(int(x.max()) for x in ref.tile_select_ref(ties.view(F32), 8, [1], 2)["n_equal"]) > 1


def test_the_rank_rule_of_the_restatement():
    want = {(1, 0, 1): 0, (1, 1, 2): 0, (1, 1, 1): 0, (9, 1, 2): 4, (9, 19, 20): 8, (9, 1, 1): 8, (63, 1, 2): 31, (64, 1, 2): 31,
            (64, 19, 20): 60, (63, 19, 20): 59, (4096, 1, 2): 2047, (4096, 19, 20): 3891, (4096, 1, 1): 4095, (4096, 65535, 65536): 4095,
            (64, 65535, 65536): 63, (9, 0, 7): 0}
    for (n, num, den), r in want.items():
        assert ref.rank_of(n, num, den) == r, (n, num, den)
        assert r == sel_ref.nearest_rank(num / den, n) or den == 65536      # the film rule, where the double q is exact enough
    assert ref.as_fraction(0.95) == (19, 20) and ref.as_fraction(0.5) == (1, 2) and ref.as_fraction((3, 7)) == (3, 7) and ref.as_fraction(1.0) == (1, 1)


def test_one_tile_over_the_film_is_score_select():
    rng = np.random.default_rng(22)
    for W, H in ((1, 1), (7, 3), (33, 64), (64, 64)):
        score = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32).view(F32)
        nums, den = [0, 1, 19, 20], 20
        t = ref.tile_select_ref(score, 64, nums, den)
        s = sel_ref.select_ref(score, [ref.rank_of(W * H, num, den) for num in nums])
        for r in range(4):
            assert t["value"][r].shape == (1, 1)
            assert (int(t["value"][r].view(np.uint32)[0, 0]), int(t["n_below"][r][0, 0]), int(t["n_equal"][r][0, 0])) == \
                   (s["value_bits"][r], s["n_below"][r], s["n_equal"][r])


def test_the_gate_restatement_equals_a_brute_force_loop():
    rng = np.random.default_rng(23)
    for (H, W), tile in (((11, 19), 8), ((5, 17), 16), ((1, 1), 8), ((33, 9), 8)):
        ty, tx = -(-H // tile), -(-W // tile)
        values = rng.choice(np.array([0, 0x3C000000, 0x3D000000, 0x7F800000, 0xFFC00000, 0x80000001], np.uint32), ty * tx)
        image = rng.integers(1, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)
        for closed in (None, rng.integers(0, 2, ty * tx).astype(np.int32) * 7):
            for thr in (0.01, 0.0, -1.0, INF):
                o, c, res, gated = ref.gate_ref(H, W, tile, values.view(F32), thr, closed, [image])
                bo, bc, bres, bg = ref.gate_brute(H, W, tile, values, sel_ref.key_of(thr), None if closed is None else closed.tolist(), image)
                assert o.reshape(-1).tolist() == bo and res == bres and gated[0].tolist() == bg
                assert (c is None and bc is None) or c.reshape(-1).tolist() == bc
                if closed is not None:
                    assert (c.reshape(-1)[closed != 0] == 7).all() and not o.reshape(-1)[closed != 0].any()      # a closed tile keeps its word


# ---------------------------------------------------------------- 2. the args header, alone
def select_call(**kw):
    c = dict(width=FW, height=FH, score=SCORE_AT, tile=TILE, q_den=20, n_ranks=4, q_given=1, given=1, q=[0, 10, 19, 20])
    c.update({"%s%d" % (f, i): plane_at(f, i) for f, i in SLOTS})
    c.update(kw)
    return c


def no_slots_from(n):
    return {"%s%d" % (f, i): 0 for f, i in SLOTS if i >= n}


def select_table():
    t = {}
    t["valid"] = select_call()
    for tile in ref.TILES:
        t["valid_tile_%d" % tile] = select_call(tile=tile)
    t["valid_one_rank"] = select_call(n_ranks=1, **no_slots_from(1))
    t["valid_two_ranks_values_only"] = select_call(n_ranks=2, **{"%s%d" % (f, i): 0 for f, i in SLOTS if i >= 2 or f != "value"})
    t["valid_one_plane_in_the_last_slot"] = select_call(**{"%s%d" % (f, i): 0 for f, i in SLOTS if (f, i) != ("n_equal", 3)})
    t["valid_largest_denominator"] = select_call(q_den=65536, q=[0, 1, 65535, 65536])
    t["valid_denominator_one"] = select_call(q_den=1, q=[0, 1, 1, 0])
    t["valid_odd_film"] = select_call(width=37, height=29)
    t["valid_one_pixel"] = select_call(width=1, height=1, tile=64)
    t["valid_unaligned_score"] = select_call(score=SCORE_AT + 4)
    t["valid_largest_film"] = select_call(width=65535, height=65535, tile=8, score=1 << 40, **{"%s%d" % (f, i): (2 + 4 * ref.FIELDS.index(f) + i) << 40 for f, i in SLOTS})
    t["valid_plane_right_behind_score"] = select_call(value0=SCORE_AT + PX)
    t["valid_planes_back_to_back"] = select_call(value1=plane_at("value", 0) + PLANE_BYTES)
    t["valid_unused_numerators_are_not_read"] = select_call(n_ranks=1, q=[20, -5, 99, 1 << 30], **no_slots_from(1))
    t["zero_width"] = select_call(width=0)
    t["zero_height"] = select_call(height=0)
    t["null_score"] = select_call(score=0)
    t["null_q_num"] = select_call(q_given=0)
    t["null_out"] = select_call(given=0)
    t["every_plane_null"] = select_call(**no_slots_from(0))
    t["plane_in_a_slot_past_n_ranks"] = select_call(n_ranks=2, **{k: v for k, v in no_slots_from(2).items() if k != "n_below3"})
    t["only_plane_in_a_slot_past_n_ranks"] = select_call(n_ranks=1, **{k: v for k, v in no_slots_from(0).items() if k != "value1"})
    t["misaligned_score"] = select_call(score=SCORE_AT + 2)
    for f, i in (("value", 0), ("n_below", 2), ("n_equal", 3)):
        t["misaligned_%s%d" % (f, i)] = select_call(**{"%s%d" % (f, i): plane_at(f, i) + 2})
    for tile in (0, -8, 4, 12, 24, 128):
        t["tile_%s" % str(tile).replace("-", "minus_")] = select_call(tile=tile)
    t["n_ranks_0"] = select_call(n_ranks=0)
    t["n_ranks_5"] = select_call(n_ranks=5)
    t["n_ranks_negative"] = select_call(n_ranks=-1)
    t["q_den_0"] = select_call(q_den=0, q=[0, 0, 0, 0])
    t["q_den_65537"] = select_call(q_den=65537)
    t["q_den_negative"] = select_call(q_den=-20)
    t["q_num_negative"] = select_call(q=[0, -1, 19, 20])
    t["q_num_above_q_den"] = select_call(q=[0, 10, 19, 21])
    t["plane_is_score"] = select_call(value2=SCORE_AT)
    t["plane_in_the_last_bytes_of_score"] = select_call(n_below0=SCORE_AT + PX - 4)
    t["plane_ends_inside_score"] = select_call(n_equal1=SCORE_AT - PLANE_BYTES + 4)
    t["two_planes_are_one"] = select_call(n_below1=plane_at("value", 3))
    t["plane_ends_inside_another"] = select_call(value1=plane_at("value", 0) + PLANE_BYTES - 4)
    # the order of the checks: each call breaks two rules, the earlier one is named
    t["order_size_before_null"] = select_call(width=0, score=0)
    t["order_null_score_before_null_q_num"] = select_call(score=0, q_given=0)
    t["order_null_q_num_before_null_out"] = select_call(q_given=0, given=0)
    t["order_null_before_every_plane_null"] = select_call(score=0, **no_slots_from(0))
    t["order_every_plane_null_before_alignment"] = select_call(score=SCORE_AT + 2, **no_slots_from(0))
    t["order_slot_before_alignment"] = select_call(n_ranks=3, score=SCORE_AT + 2)
    t["order_score_alignment_before_plane_alignment"] = select_call(score=SCORE_AT + 2, value0=plane_at("value", 0) + 1)
    t["order_plane_alignment_before_tile"] = select_call(n_equal0=plane_at("n_equal", 0) + 2, tile=5)
    t["order_tile_before_n_ranks"] = select_call(tile=5, n_ranks=9)
    t["order_n_ranks_before_q_den"] = select_call(n_ranks=0, q_den=0)
    t["order_q_den_before_q_num"] = select_call(q_den=0, q=[1, 1, 1, 1])
    t["order_q_num_before_overlap"] = select_call(q=[21, 0, 0, 0], value0=SCORE_AT)
    t["order_score_overlap_before_plane_overlap"] = select_call(value1=plane_at("value", 2), value0=SCORE_AT)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def select_restated(c):
    """include/statmc.h's error list of statmc_score_tile_select, in its order: None for a valid call, else words of the message"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    if c["score"] == 0:
        return ["null score"]
    if not c["q_given"]:
        return ["null q_num"]
    if not c["given"]:
        return ["null out"]
    if all(c["%s%d" % s] == 0 for s in SLOTS):
        return ["every plane"]
    if 1 <= c["n_ranks"] <= 4:
        for f, i in SLOTS:
            if c["%s%d" % (f, i)] and i >= c["n_ranks"]:
                return ["out->%s[%d] is given" % (f, i)]
    if c["score"] % 4:
        return ["score", "aligned"]
    for f, i in SLOTS:
        if c["%s%d" % (f, i)] % 4:
            return ["out->%s[%d] is not 4-byte aligned" % (f, i)]
    if c["tile"] not in ref.TILES:
        return ["tile = %d" % c["tile"]]
    if not 1 <= c["n_ranks"] <= 4:
        return ["n_ranks = %d" % c["n_ranks"]]
    if not 1 <= c["q_den"] <= 65536:
        return ["q_den = %d" % c["q_den"]]
    for i in range(c["n_ranks"]):
        if not 0 <= c["q"][i] <= c["q_den"]:
            return ["q_num[%d] = %d" % (i, c["q"][i])]
    px = c["width"] * c["height"] * 4
    n = -(-c["width"] // c["tile"]) * -(-c["height"] // c["tile"]) * 4
    for a, (f, i) in enumerate(SLOTS):
        if overlap(c["%s%d" % (f, i)], n, c["score"], px):
            return ["out->%s[%d] overlaps score" % (f, i)]
        for g, j in SLOTS[:a]:
            if overlap(c["%s%d" % (f, i)], n, c["%s%d" % (g, j)], n):
                return ["out->%s[%d] overlaps out->%s[%d]" % (f, i, g, j)]
    return None


GATE_AT = dict(tile_value=2 * 16 * MIB, closed=3 * 16 * MIB, open=4 * 16 * MIB, result=5 * 16 * MIB)
IMG_AT = [(8 + i) * 16 * MIB for i in range(8)]


def gate_call(**kw):
    c = dict(width=FW, height=FH, tile=TILE, threshold=f32_bits(0.02), n_images=2, src_given=1, dst_given=1,
             src=[IMG_AT[0], IMG_AT[1], 0, 0], dst=[IMG_AT[0], IMG_AT[5], 0, 0], **GATE_AT)
    c.update(kw)
    return c


def gate_table():
    t = {}
    t["gate_valid"] = gate_call()
    for tile in ref.TILES:
        t["gate_valid_tile_%d" % tile] = gate_call(tile=tile)
    t["gate_valid_no_images"] = gate_call(n_images=0, src_given=0, dst_given=0)
    t["gate_valid_no_closed_no_result"] = gate_call(closed=0, result=0)
    t["gate_valid_four_images_in_place"] = gate_call(n_images=4, src=IMG_AT[:4], dst=IMG_AT[:4])
    t["gate_valid_four_images_out_of_place"] = gate_call(n_images=4, src=IMG_AT[:4], dst=IMG_AT[4:])
    t["gate_valid_two_images_share_a_source"] = gate_call(src=[IMG_AT[0], IMG_AT[0], 0, 0], dst=[IMG_AT[4], IMG_AT[5], 0, 0])
    t["gate_valid_unaligned_image"] = gate_call(src=[IMG_AT[0] + 4, IMG_AT[1], 0, 0], dst=[IMG_AT[0] + 4, IMG_AT[5], 0, 0])
    t["gate_valid_negative_and_infinite_thresholds_0"] = gate_call(threshold=f32_bits(-1.0))
    t["gate_valid_negative_and_infinite_thresholds_1"] = gate_call(threshold=f32_bits(INF))
    t["gate_valid_planes_back_to_back"] = gate_call(open=GATE_AT["closed"] + PLANE_BYTES)
    t["gate_valid_largest_film"] = gate_call(width=65535, height=65535, tile=8, tile_value=1 << 40, closed=2 << 40, open=3 << 40, result=4 << 40,
                                             src=[5 << 40, 6 << 40, 0, 0], dst=[5 << 40, 7 << 40, 0, 0])
    t["gate_zero_width"] = gate_call(width=0)
    t["gate_zero_height"] = gate_call(height=0)
    t["gate_null_tile_value"] = gate_call(tile_value=0)
    t["gate_null_open"] = gate_call(open=0)
    t["gate_n_images_5"] = gate_call(n_images=5)
    t["gate_n_images_negative"] = gate_call(n_images=-1)
    t["gate_null_src"] = gate_call(src_given=0)
    t["gate_null_dst"] = gate_call(dst_given=0)
    t["gate_null_source_image"] = gate_call(src=[IMG_AT[0], 0, 0, 0])
    t["gate_null_destination_image"] = gate_call(dst=[0, IMG_AT[5], 0, 0])
    for name in ("tile_value", "closed", "open"):
        t["gate_misaligned_" + name] = gate_call(**{name: GATE_AT[name] + 2})
    t["gate_misaligned_source"] = gate_call(src=[IMG_AT[0], IMG_AT[1] + 1, 0, 0])
    t["gate_misaligned_destination"] = gate_call(dst=[IMG_AT[0], IMG_AT[5] + 2, 0, 0])
    t["gate_misaligned_result"] = gate_call(result=GATE_AT["result"] + 4)
    for tile in (0, 4, 24, 128):
        t["gate_tile_%d" % tile] = gate_call(tile=tile)
    for i, b in enumerate(NAN_BITS):
        t["gate_nan_threshold_%d" % i] = gate_call(threshold=b)
    t["gate_open_is_tile_value"] = gate_call(open=GATE_AT["tile_value"])
    t["gate_closed_is_open"] = gate_call(closed=GATE_AT["open"])
    t["gate_closed_ends_inside_tile_value"] = gate_call(closed=GATE_AT["tile_value"] - PLANE_BYTES + 4)
    t["gate_result_in_open"] = gate_call(result=GATE_AT["open"] + 8)
    t["gate_destination_shifted_over_its_source"] = gate_call(dst=[IMG_AT[0] + 16, IMG_AT[5], 0, 0])
    t["gate_source_over_open"] = gate_call(src=[IMG_AT[0], GATE_AT["open"] - PX + 4, 0, 0])
    t["gate_destination_over_result"] = gate_call(dst=[IMG_AT[0], GATE_AT["result"] - 4, 0, 0])
    t["gate_destination_over_tile_value"] = gate_call(dst=[IMG_AT[0], GATE_AT["tile_value"], 0, 0])
    t["gate_destination_is_another_source"] = gate_call(src=[IMG_AT[0], IMG_AT[1], 0, 0], dst=[IMG_AT[4], IMG_AT[0], 0, 0])
    t["gate_two_destinations_are_one"] = gate_call(src=[IMG_AT[0], IMG_AT[1], 0, 0], dst=[IMG_AT[4], IMG_AT[4], 0, 0])
    t["gate_order_size_before_null"] = gate_call(width=0, tile_value=0)
    t["gate_order_null_tile_value_before_null_open"] = gate_call(tile_value=0, open=0)
    t["gate_order_null_before_n_images"] = gate_call(open=0, n_images=7)
    t["gate_order_n_images_before_null_src"] = gate_call(n_images=9, src_given=0)
    t["gate_order_null_src_before_null_dst"] = gate_call(src_given=0, dst_given=0)
    t["gate_order_null_image_before_alignment"] = gate_call(src=[IMG_AT[0], 0, 0, 0], tile_value=GATE_AT["tile_value"] + 2)
    t["gate_order_plane_alignment_before_image_alignment"] = gate_call(open=GATE_AT["open"] + 2, src=[IMG_AT[0] + 2, IMG_AT[1], 0, 0])
    t["gate_order_image_alignment_before_result_alignment"] = gate_call(dst=[IMG_AT[0], IMG_AT[5] + 2, 0, 0], result=GATE_AT["result"] + 4)
    t["gate_order_alignment_before_tile"] = gate_call(result=GATE_AT["result"] + 4, tile=5)
    t["gate_order_tile_before_nan"] = gate_call(tile=5, threshold=NAN_BITS[0])
    t["gate_order_nan_before_overlap"] = gate_call(threshold=NAN_BITS[1], open=GATE_AT["tile_value"])
    t["gate_order_plane_overlap_before_image_overlap"] = gate_call(closed=GATE_AT["open"], dst=[IMG_AT[0] + 16, IMG_AT[5], 0, 0])
    return t


def gate_restated(c):
    """include/statmc.h's error list of statmc_gate_tiles, in its order"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    if c["tile_value"] == 0:
        return ["null tile_value"]
    if c["open"] == 0:
        return ["null open"]
    k = c["n_images"]
    if not 0 <= k <= 4:
        return ["n_images = %d" % k]
    if k and not c["src_given"]:
        return ["null src"]
    if k and not c["dst_given"]:
        return ["null dst"]
    for i in range(k):
        if c["src"][i] == 0:
            return ["null src[%d]" % i]
        if c["dst"][i] == 0:
            return ["null dst[%d]" % i]
    for name in ("tile_value", "closed", "open"):
        if c[name] % 4:
            return [name + " is not 4-byte aligned"]
    for i in range(k):
        if c["src"][i] % 4:
            return ["src[%d] is not 4-byte aligned" % i]
        if c["dst"][i] % 4:
            return ["dst[%d] is not 4-byte aligned" % i]
    if c["result"] % 8:
        return ["result is not 8-byte aligned"]
    if c["tile"] not in ref.TILES:
        return ["tile = %d" % c["tile"]]
    if (c["threshold"] & 0x7FFFFFFF) > 0x7F800000:
        return ["threshold", "NaN"]
    px = c["width"] * c["height"] * 4
    n = -(-c["width"] // c["tile"]) * -(-c["height"] // c["tile"]) * 4
    small = [("tile_value", n), ("closed", n), ("open", n), ("result", 32)]
    for a, (p, np_) in enumerate(small):
        for q, nq in small[:a]:
            if overlap(c[p], np_, c[q], nq):
                return ["%s overlaps %s" % (p, q)]
    for i in range(k):
        if c["src"][i] != c["dst"][i] and overlap(c["src"][i], px, c["dst"][i], px):
            return ["dst[%d] overlaps src[%d] without being equal" % (i, i)]
        for p, np_ in small:
            if overlap(c["src"][i], px, c[p], np_):
                return ["src[%d] overlaps %s" % (i, p)]
            if overlap(c["dst"][i], px, c[p], np_):
                return ["dst[%d] overlaps %s" % (i, p)]
        for j in range(k):
            if j == i:
                continue
            if overlap(c["dst"][i], px, c["src"][j], px):
                return ["dst[%d] overlaps src[%d]" % (i, j)]
            if j < i and overlap(c["dst"][i], px, c["dst"][j], px):
                return ["dst[%d] overlaps dst[%d]" % (i, j)]
    return None


RANK_NS = (1, 9, 63, 64, 4096)
RANK_QS = ((0, 1), (1, 2), (19, 20), (1, 1), (65535, 65536))


def films():
    """whole selects for the host: (float bits [H][W], tile, nums, den)"""
    rng = np.random.default_rng(6)
    f = {}
    every = rng.integers(0, 2 ** 32, (37, 29), dtype=np.uint64).astype(np.uint32)
    every[0, :6] = [0x7FC00000, 0xFFC00000, 0x80000000, 0xFF800000, 0x7F800000, 1]
    for tile in ref.TILES:
        f["film_random_bits_%d" % tile] = (every, tile, [0, 10, 19, 20], 20)
    f["film_random_bits_one_rank"] = (every, 8, [1], 2)
    f["film_random_bits_largest_denominator"] = (every, 16, [1, 65535, 65536], 65536)
    ties = rng.choice(np.array([0, 1, 0x3F800000, 0x7F800000], np.uint32), (20, 70))
    f["film_ties"] = (ties, 8, [0, 1, 3, 4], 4)
    for name, b in (("one", 0x3F800000), ("smallest_subnormal", 1), ("infinite", 0x7F800000), ("zero", 0), ("nan", 0xFFC00000)):
        f["film_constant_" + name] = (np.full((70, 67), b, np.uint32), 64, [0, 1, 2], 2)
    f["film_one_pixel"] = (np.array([[0x7F7FFFFF]], np.uint32), 8, [0, 1], 1)
    return f


def gate_films():
    """whole tile passes for the host: (H, W, tile, threshold bits, tile value bits, closed or None)"""
    rng = np.random.default_rng(7)
    g = {}
    for name, (H, W, tile) in (("gatefilm_odd", (37, 29, 8)), ("gatefilm_one_tile", (5, 5, 64)), ("gatefilm_wide", (16, 257, 16))):
        n = -(-H // tile) * -(-W // tile)
        values = rng.choice(np.array([0, 0x3C000000, 0x3CA3D70A, 0x3D000000, 0x7F800000, 0xFFC00000, 0x80000001], np.uint32), n)
        g[name] = (H, W, tile, f32_bits(0.02), values, None)
        g[name + "_with_memory"] = (H, W, tile, f32_bits(0.02), values, rng.integers(0, 2, n).astype(np.int32) * 5)
        g[name + "_negative_threshold"] = (H, W, tile, f32_bits(-3.0), values, np.zeros(n, np.int32))
    return g


def write_table(path):
    with open(path, "w") as f:
        for name, c in select_table().items():
            f.write("select %s %d %d %d %d %d %d %d %d %s %s\n" % (name, c["width"], c["height"], c["score"], c["tile"], c["q_den"], c["n_ranks"], c["q_given"],
                                                                  c["given"], " ".join(str(q) for q in c["q"]), " ".join(str(c["%s%d" % s]) for s in SLOTS)))
        for name, c in gate_table().items():
            f.write("gate %s %d %d %d %d %d %d %d %d %d %d %s %s %d\n" % (name, c["width"], c["height"], c["tile"], c["tile_value"], c["threshold"], c["closed"],
                                                                       c["open"], c["n_images"], c["src_given"], c["dst_given"],
                                                                       " ".join(map(str, c["src"])), " ".join(map(str, c["dst"])), c["result"]))
        for n in RANK_NS:
            for num, den in RANK_QS:
                f.write("rank rank_%d_%d_%d %d %d %d\n" % (n, num, den, n, num, den))
        for name, (bits, tile, nums, den) in films().items():
            f.write("film %s %d %d %d %d %d %s %s\n" % (name, bits.shape[1], bits.shape[0], tile, den, len(nums), " ".join(str(q) for q in (nums + [0] * 4)[:4]),
                                                       " ".join(str(int(b)) for b in bits.reshape(-1))))
        for name, (H, W, tile, thr, values, closed) in gate_films().items():
            f.write("gatefilm %s %d %d %d %d %d %s %s\n" % (name, W, H, tile, thr, closed is not None, " ".join(str(int(v)) for v in values),
                                                           "" if closed is None else " ".join(str(int(v)) for v in closed)))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("tile_select") / "table.txt")
    write_table(path)
    out = verdicts(build.TILE_SELECT_ARGS_BIN, path)
    return path, out, dict(line.split(" : ", 1) for line in out.splitlines())


def test_the_tables_state_every_error_and_valid_calls():
    for table, restated, prefix in ((select_table(), select_restated, "valid"), (gate_table(), gate_restated, "gate_valid")):
        want = {name: restated(c) for name, c in table.items()}
        for name, w in want.items():
            assert (w is None) == name.startswith(prefix), (name, w)
        said = set(re.sub(r"\[\d\]|= -?\d+", "", " ".join(w)) for w in want.values() if w)
        assert len(said) >= 14, sorted(said)
    s = {name: select_restated(c) for name, c in select_table().items()}
    assert s["order_size_before_null"] == ["width", "height"] and s["order_null_score_before_null_q_num"] == ["null score"]
    assert s["order_null_q_num_before_null_out"] == ["null q_num"] and s["order_null_before_every_plane_null"] == ["null score"]
    assert s["order_every_plane_null_before_alignment"] == ["every plane"] and s["order_slot_before_alignment"] == ["out->value[3] is given"]
    assert s["order_score_alignment_before_plane_alignment"] == ["score", "aligned"] and s["order_plane_alignment_before_tile"][0].startswith("out->n_equal[0]")
    assert s["order_tile_before_n_ranks"] == ["tile = 5"] and s["order_n_ranks_before_q_den"] == ["n_ranks = 0"] and s["order_q_den_before_q_num"] == ["q_den = 0"]
    assert s["order_q_num_before_overlap"] == ["q_num[0] = 21"] and s["order_score_overlap_before_plane_overlap"] == ["out->value[0] overlaps score"]
    assert s["only_plane_in_a_slot_past_n_ranks"] == ["out->value[1] is given"] and s["two_planes_are_one"] == ["out->n_below[1] overlaps out->value[3]"]
    g = {name: gate_restated(c) for name, c in gate_table().items()}
    assert g["gate_order_null_before_n_images"] == ["null open"] and g["gate_order_n_images_before_null_src"] == ["n_images = 9"]
    assert g["gate_order_null_src_before_null_dst"] == ["null src"] and g["gate_order_null_image_before_alignment"] == ["null src[1]"]
    assert g["gate_order_plane_alignment_before_image_alignment"] == ["open is not 4-byte aligned"]
    assert g["gate_order_image_alignment_before_result_alignment"] == ["dst[1] is not 4-byte aligned"] and g["gate_order_alignment_before_tile"] == ["result is not 8-byte aligned"]
    assert g["gate_order_tile_before_nan"] == ["tile = 5"] and g["gate_order_nan_before_overlap"] == ["threshold", "NaN"]
    assert g["gate_order_plane_overlap_before_image_overlap"] == ["open overlaps closed"]
    assert g["gate_destination_is_another_source"] == ["dst[1] overlaps src[0]"] and g["gate_two_destinations_are_one"] == ["dst[1] overlaps dst[0]"]
    assert g["gate_source_over_open"] == ["src[1] overlaps open"] and g["gate_destination_over_result"] == ["dst[1] overlaps result"]


SELECT_NAMES = ["score", "tile", "q_num", "q_den", "n_ranks", "width"] + ["out->" + f for f in ref.FIELDS]
GATE_NAMES = ["tile_value", "closed", "open", "result", "threshold", "tile", "n_images", "width", "src", "dst"]


def test_the_args_program_gives_the_restated_verdicts(args_out):
    _, out, got = args_out
    assert sorted(got) == sorted(list(select_table()) + list(gate_table()) + list(films()) + list(gate_films()) +
                                 ["rank_%d_%d_%d" % (n, num, den) for n in RANK_NS for num, den in RANK_QS])
    for table, restated, names in ((select_table(), select_restated, SELECT_NAMES), (gate_table(), gate_restated, GATE_NAMES)):
        for name, c in table.items():
            want = restated(c)
            tx, ty = (-(-c["width"] // c["tile"]), -(-c["height"] // c["tile"])) if want is None else (0, 0)
            if want is not None:
                assert not got[name].startswith("ok"), (name, got[name])
                for word in want:
                    assert word in got[name], (name, word, got[name])
                for other in names:
                    if not any(other in w for w in want):      # only the argument at fault is named
                        if other == "n_ranks" and "is given" in got[name]:
                            continue      # "slots n_ranks .. 3 must be null" is said in numbers
                        assert not re.search(r"(?<![\w>])%s\b" % re.escape(other), got[name]), (name, other, got[name])
            elif "q" in c:
                assert got[name] == "ok select %d %d %d %d" % (tx, ty, tx * ty, int(c["score"] % 16 == 0)), (name, got[name])
            else:
                vec = all(p % 16 == 0 for p in c["src"][:c["n_images"]] + c["dst"][:c["n_images"]])
                assert got[name] == "ok gate %d %d %d %08x %d %d" % (tx, ty, tx * ty, sel_ref.key_of(bits_f32(c["threshold"])),
                                                                    {8: 3, 16: 4, 32: 5, 64: 6}[c["tile"]], int(vec)), (name, got[name])
    assert got["valid_largest_film"].split()[2:5] == ["8192", "8192", str(8192 * 8192)]
    assert got["gate_valid_negative_and_infinite_thresholds_0"].split()[5] == "00000000"


def test_the_rank_rule_in_the_header(args_out):
    _, _, got = args_out
    for n in RANK_NS:
        for num, den in RANK_QS:
            assert got["rank_%d_%d_%d" % (n, num, den)] == "rank %d" % ref.rank_of(n, num, den)
    assert got["rank_4096_19_20"] == "rank 3891" and got["rank_1_0_1"] == "rank 0" and got["rank_64_1_2"] == "rank 31" and got["rank_4096_65535_65536"] == "rank 4095"


def test_whole_films_on_the_host_equal_the_restatement_bit_for_bit(args_out):
    _, _, got = args_out
    for name, (bits, tile, nums, den) in films().items():
        w = ref.tile_select_ref(bits.view(F32), tile, nums, den)
        ty, tx = w["value"][0].shape
        want = "film %d %d" % (tx, ty)
        for j in range(ty):
            for i in range(tx):
                for r in range(len(nums)):
                    want += " %08x %d %d" % (int(w["value"][r].view(np.uint32)[j, i]), w["n_below"][r][j, i], w["n_equal"][r][j, i])
        assert got[name] == want, name
    assert got["film_constant_infinite"].split()[3:6] == ["7f800000", "0", "4096"] and got["film_constant_nan"].split()[3:6] == ["00000000", "0", "4096"]
    for name, (H, W, tile, thr, values, closed) in gate_films().items():
        o, c, res, _ = ref.gate_ref(H, W, tile, values.view(F32), float(bits_f32(thr)), closed, [])
        want = "gatefilm %d %d %d %d" % (res["n_tiles"], res["n_open"], res["n_closed_now"], res["n_px_open"])
        for t in range(o.size):
            want += " %d/%d" % (o.reshape(-1)[t], -1 if c is None else c.reshape(-1)[t])
        assert got[name] == want, name


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain, _ = args_out
    binary = str(tmp_path / "tile_select_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


def test_the_args_header_compiles_with_nothing_but_the_c_header(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "%s"\nint main() { return statmc::tile_select_rank(64, 19, 20) == 60 && statmc::tile_pixels(9, 9, 8, 1, 1) == 1 ? 0 : 1; }\n' % ARGS_HEADER)
    binary = str(tmp_path / "alone")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-nostdinc++", "-fsyntax-only", "-x", "c++", str(src)])      # no C++ library header at all
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", binary])
    assert subprocess.run([binary]).returncode == 0
    text = re.sub(r"//.*", "", open(ARGS_HEADER).read())
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|\basm\b|__host__|__device__", text)      # no HIP call, type or kernel, no inline assembly
    assert re.findall(r'#include "([^"]+)"', text) == ["statmc_score_tiles_args.h"]


# ---------------------------------------------------------------- 3. the library, without a device
def test_the_symbols_are_exported_declared_and_mirrored(lib, tmp_path):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    for name in ("statmc_score_tile_select", "statmc_gate_tiles"):
        assert hasattr(lib, name) and name in api.EXPORTS
    decl = re.search(r"int statmc_score_tile_select\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, const float *score, int tile, const int32_t *q_num, "
                                                       "int32_t q_den, int n_ranks, const statmc_tile_quantiles *out, void *stream")
    decl = re.search(r"int statmc_gate_tiles\s*\(([^;]*)\)\s*;", header)
    assert decl and " ".join(re.sub(r"/\*.*?\*/", "", decl.group(1)).split()) == (
        "uint16_t width, uint16_t height, int tile, const float *tile_value, float threshold, int32_t *closed, int32_t *open, "
        "const void *const *src, void *const *dst, int n_images, statmc_gate_result *result, void *stream")
    assert re.search(r"#define STATMC_TILE_SELECT_MAX_RANKS 4\b", header) and api.TILE_SELECT_MAX_RANKS == ref.MAX_RANKS == 4
    assert re.search(r"#define STATMC_GATE_MAX_IMAGES 4\b", header) and api.GATE_MAX_IMAGES == 4 and api.TILE_SELECT_MAX_DEN == ref.MAX_DEN
    names = [f for f, _ in api.TileQuantiles._fields_]
    assert tuple(names) == api.TILE_QUANTILE_FIELDS == ref.FIELDS
    gate_names = [f for f, _ in api.GateResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "statmc.h"\nint main(void) {\n  printf("%zu", sizeof(statmc_tile_quantiles));\n'
                   + "".join('  printf(" %%zu", offsetof(statmc_tile_quantiles, %s));\n' % f for f in names)
                   + '  printf(" %zu", sizeof(statmc_gate_result));\n'
                   + "".join('  printf(" %%zu", offsetof(statmc_gate_result, %s));\n' % f for f in gate_names) + "  return 0;\n}\n")
    binary = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", binary])
    got = [int(x) for x in subprocess.check_output([binary]).split()]
    tq, gr = api.TileQuantiles, api.GateResult
    assert got == [C.sizeof(tq)] + [getattr(tq, f).offset for f in names] + [C.sizeof(gr)] + [getattr(gr, f).offset for f in gate_names]
    assert got == [96, 0, 32, 64, 32, 0, 8, 16, 24]
    assert "statmc_tile_select.hip" in build.SOURCES and "statmc_tile_select_args.h" in build.HEADERS and build.TILE_SELECT_ARGS_BIN in build.TOOLS
    assert all(callable(f) for f in (api.score_tile_select, api.read_tile_quantiles, api.gate_tiles, api.read_gate_result,
                                     film.FilmStats.score_tile_quantiles, film.FilmStats.gate_tiles))
    assert api.tile_quantile_fraction(0.95) == (19, 20) and api.tile_quantile_fraction((3, 4)) == (3, 4) and api.tile_quantile_fraction(0.0) == (0, 1)
    kernel = re.sub(r"//.*", "", open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_tile_select.hip")).read())
    assert not re.search(r"\basm\b|hipMalloc|hipMemcpy", kernel) and len(re.findall(r"hipMemsetAsync", kernel)) == 1      # only the gate's result is zeroed


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up image pointers, never dereferenced; out, q_num, src and dst are real host memory.  Every invalid call of the tables is
    refused with its argument named whether or not a device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in select_table().items():
        want = select_restated(c)
        out = api.TileQuantiles()
        for f, i in SLOTS:
            getattr(out, f)[i] = c["%s%d" % (f, i)] or None
        q = (C.c_int32 * 4)(*c["q"])
        run = lambda: lib.statmc_score_tile_select(c["width"], c["height"], c["score"] or None, c["tile"], q if c["q_given"] else None, c["q_den"],
                                                   c["n_ranks"], C.byref(out) if c["given"] else None, None)
        if want is not None:
            assert run() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_tile_select_gpu.py runs real ones)
            assert run() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()
    for name, c in gate_table().items():
        want = gate_restated(c)
        src, dst = (C.c_void_p * 4)(*[p or None for p in c["src"]]), (C.c_void_p * 4)(*[p or None for p in c["dst"]])
        thr = C.c_float()
        C.memmove(C.byref(thr), C.byref(C.c_uint32(c["threshold"])), 4)      # the bits as they are, NaN payloads too
        run = lambda: lib.statmc_gate_tiles(c["width"], c["height"], c["tile"], c["tile_value"] or None, thr, c["closed"] or None, c["open"] or None,
                                            src if c["src_given"] else None, dst if c["dst_given"] else None, c["n_images"], c["result"] or None, None)
        if want is not None:
            assert run() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():
            assert run() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()
