"""statmc_score_tile_select and statmc_gate_tiles (include/statmc.h) restated in numpy: per tile np.sort of the keys and the entry at
the nearest rank, the counts by comparison; the gate as boolean planes and np.repeat of the open plane over the pixels.  Nothing of
the library is used."""
from fractions import Fraction

import numpy as np

from score_sum_reference import key_of, keys_of

TILES = (8, 16, 32, 64)
MAX_RANKS = 4
MAX_DEN = 65536
FIELDS = ("value", "n_below", "n_equal")
NO_KEY = np.uint32(0xFFFFFFFF)      # pads a partial tile: above every key, never at a rank below n


def rank_of(n, num, den):
    """the 0-based nearest rank of quantile num / den among n sorted keys: max(0, ceil(n num / den) - 1), in integers"""
    assert n >= 1 and 1 <= den <= MAX_DEN and 0 <= num <= den
    return max(0, -(-n * num // den) - 1)


def as_fraction(q):
    """(num, den) of a quantile given as a pair or as a float: a float goes through Fraction(q).limit_denominator(65536)"""
    if isinstance(q, (tuple, list)):
        return int(q[0]), int(q[1])
    f = Fraction(q).limit_denominator(MAX_DEN)
    return f.numerator, f.denominator


def tile_blocks(keys, tile):
    """keys [H][W] as [tiles_y][tiles_x][tile * tile], partial tiles padded with NO_KEY, and the pixel counts [tiles_y][tiles_x]"""
    H, W = keys.shape
    ty, tx = -(-H // tile), -(-W // tile)
    padded = np.full((ty * tile, tx * tile), NO_KEY, np.uint32)
    padded[:H, :W] = keys
    blocks = padded.reshape(ty, tile, tx, tile).transpose(0, 2, 1, 3).reshape(ty, tx, tile * tile)
    hs = np.minimum(tile, H - tile * np.arange(ty))
    ws = np.minimum(tile, W - tile * np.arange(tx))
    return blocks, (hs[:, None] * ws[None, :]).astype(np.int64)


def tile_select_ref(score, tile, nums, den):
    """the planes of statmc_score_tile_select for the float32 image score[H][W]: {"value": [float32 [ty][tx] per rank],
    "n_below": [int32 ...], "n_equal": [int32 ...], "rank": [int64 ...]}"""
    assert tile in TILES and 1 <= len(nums) <= MAX_RANKS
    score = np.asarray(score, np.float32)
    H, W = score.shape
    blocks, n = tile_blocks(keys_of(score).reshape(H, W), tile)
    ordered = np.sort(blocks, axis=-1)
    out = {f: [] for f in FIELDS + ("rank",)}
    for num in nums:
        rank = np.maximum(0, -(-n * int(num) // int(den)) - 1)
        assert int(n.max()) * int(num) <= 1 << 28
        v = np.take_along_axis(ordered, rank[..., None], axis=-1)[..., 0]
        assert not (v == NO_KEY).any()
        out["value"].append(v.view(np.float32))
        out["n_below"].append((blocks < v[..., None]).sum(-1).astype(np.int32))
        out["n_equal"].append((blocks == v[..., None]).sum(-1).astype(np.int32))
        out["rank"].append(rank)
    return out


def tile_select_brute(score, tile, nums, den):
    """the same a tile and a pixel at a time in Python integers: {(ty, tx, i): (value bits, n_below, n_equal)}"""
    bits = np.asarray(score, np.float32).view(np.uint32)
    H, W = bits.shape
    out = {}
    for j in range(-(-H // tile)):
        for i in range(-(-W // tile)):
            keys = []
            for y in range(j * tile, min((j + 1) * tile, H)):
                for x in range(i * tile, min((i + 1) * tile, W)):
                    b = int(bits[y, x])
                    keys.append(0 if (b & 0x7FFFFFFF) > 0x7F800000 or b >> 31 else b)
            keys.sort()
            for r, num in enumerate(nums):
                v = keys[rank_of(len(keys), num, den)]
                out[(j, i, r)] = (v, sum(k < v for k in keys), sum(k == v for k in keys))
    return out


def tile_of_pixels(H, W, tile):
    """the tile index ty * tiles_x + tx of every pixel, [H][W]"""
    tx = -(-W // tile)
    return (np.arange(H)[:, None] // tile) * tx + np.arange(W)[None, :] // tile


def gate_ref(H, W, tile, tile_value, threshold, closed, images):
    """statmc_gate_tiles: (open int32 [ty][tx], the new closed plane or None, result dict, the gated images as uint32 words).
    `closed` is an int32 plane or None; `images` a list of [H][W] arrays of 32-bit words (any 4-byte dtype)."""
    assert tile in TILES
    ty, tx = -(-H // tile), -(-W // tile)
    tile_value = np.asarray(tile_value, np.float32).reshape(ty, tx)
    above = keys_of(tile_value).reshape(ty, tx) > np.uint32(key_of(threshold))
    was_closed = np.zeros((ty, tx), bool) if closed is None else np.asarray(closed).reshape(ty, tx) != 0
    is_open = ~was_closed & above
    new_closed = None
    if closed is not None:
        new_closed = np.where(was_closed, np.asarray(closed, np.int32).reshape(ty, tx), np.where(above, 0, 1)).astype(np.int32)
    hs = np.minimum(tile, H - tile * np.arange(ty))
    ws = np.minimum(tile, W - tile * np.arange(tx))
    n_px = hs[:, None] * ws[None, :]
    result = {"n_tiles": ty * tx, "n_open": int(is_open.sum()), "n_closed_now": int((~was_closed & ~above).sum()),
              "n_px_open": int(n_px[is_open].sum())}
    keep = is_open.reshape(-1)[tile_of_pixels(H, W, tile)]
    gated = [np.where(keep, np.ascontiguousarray(im).view(np.uint32).reshape(H, W), np.uint32(0)) for im in images]
    return is_open.astype(np.int32), new_closed, result, gated


def gate_brute(H, W, tile, tile_value_bits, threshold_key, closed, image_words):
    """the gate a tile and a pixel at a time in Python: (open list, closed list or None, result dict, gated image as a list of rows)"""
    ty, tx = -(-H // tile), -(-W // tile)
    is_open, new_closed, res = [], None if closed is None else list(closed), {"n_tiles": ty * tx, "n_open": 0, "n_closed_now": 0, "n_px_open": 0}
    for t in range(ty * tx):
        b = int(tile_value_bits[t])
        k = 0 if (b & 0x7FFFFFFF) > 0x7F800000 or b >> 31 else b
        was = closed is not None and closed[t] != 0
        above = k > threshold_key
        is_open.append(int(not was and above))
        if closed is not None and not was:
            new_closed[t] = 0 if above else 1
        res["n_open"] += is_open[-1]
        res["n_closed_now"] += int(not was and not above)
    gated = [[0] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            t = (y // tile) * tx + x // tile
            if is_open[t]:
                res["n_px_open"] += 1
                gated[y][x] = int(image_words[y][x])
    return is_open, new_closed, res, gated
