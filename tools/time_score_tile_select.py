"""Times statmc_score_tile_select and statmc_gate_tiles at 1920 x 1080 and 3840 x 2160, in one process, against the library's other
ways to the same answer:

  tile_select     tile 8, 16, 32 and 64; one rank (19/20) and four (0, 1/2, 19/20, 1), all three planes of every rank, on
                    random_exponent   every exponent equally likely: the descent branches at every bit
                    error_scores      statmc_error_scores of random statistics, 2 to 9 samples per pixel, some below 2 (+inf)
                    constant          one score everywhere
  score_tiles     statmc_score_tiles, mean + max + n_clipped (a tile rule's three) under a cap of 0.05, same tile sizes and images
  score_select    whole-film statmc_score_select with one rank on the same three images: what one call per tile would cost, once
  host            the error-score image downloaded and np.partition per tile at one rank (a fifth of the calls: it takes far longer)
  gate_tiles      tile 16 on the 19/20 plane of the error scores at its median, one and two images out of place, against
  floor           one read of `score` (4 B/px) -- for the gate one read and one write per image (8 B/px) -- at the copy bandwidth
                  measured in the same process (a device-to-device copy of 512 MiB: bytes read plus bytes written over its time)

Nothing is reported unless every timed tile_select and gate_tiles configuration equals the numpy restatement
(tests/tile_select_reference.py) bit for bit.  One JSON line per (size, candidate): milliseconds per call (hipEvent timing, 50 calls
after 10, five alternating rounds: every round times every candidate once; mean over the rounds, and the runs), spread = max - min
over the rounds.

    python tools/time_score_tile_select.py [--iters 50 --warmup 10 --rounds 5] [--sizes 1920x1080,3840x2160] [--out profiles/score_tile_select.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tile_select_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402
from time_score_sum import copy_bandwidth, images, timed  # noqa: E402

CAP = 0.05
RULE = ("mean", "max", "n_clipped")
DEN = 20
RANKS = {1: [19], 4: [0, 10, 19, 20]}
GATE_TILE = 16      # the gate's threshold is the median of the plane it reads: about half the tiles close


def same(got, want, n):
    for f in ref.FIELDS:
        for i in range(n):
            g, w = got[f][i], want[f][i]
            if g.shape != w.shape or not np.array_equal(g.view(np.uint32) if f == "value" else g, w.view(np.uint32) if f == "value" else w):
                return False
    return True


def host_quantile(img, tile, num, den):
    """download + numpy: the value plane of one rank"""
    score = img.cpu().numpy()
    H, W = score.shape
    blocks, n = ref.tile_blocks(ref.keys_of(score).reshape(H, W), tile)
    rank = np.maximum(0, -(-n * num // den) - 1)      # at most four distinct ones: full tiles, the right edge, the bottom edge, the corner
    part = np.partition(blocks, np.unique(rank).tolist(), axis=-1)
    return np.take_along_axis(part, rank[..., None], axis=-1)[..., 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score_tile_select.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    bw = copy_bandwidth(dev, 20, 3)
    lines = [json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})]
    for W, H in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        px = W * H
        imgs = images(W, H, dev, gen)
        tile_dtypes = {"mean": torch.float32, "max": torch.float32, "n_clipped": torch.int32}
        ws = torch.empty(api.score_select_workspace(), dtype=torch.uint8, device=dev)
        result = torch.zeros(32, dtype=torch.int64, device=dev)
        cands, slow = {}, set()
        for tile in ref.TILES:
            grid = api.tile_grid(H, W, tile)
            out = {f: [torch.empty(grid, dtype=torch.float32 if f == "value" else torch.int32, device=dev) for _ in range(4)] for f in ref.FIELDS}
            rule_out = {p: torch.empty(grid, dtype=tile_dtypes[p], device=dev) for p in RULE}
            for name, img in imgs.items():
                for k, nums in RANKS.items():
                    cands["tile_select_%d_%d_%s" % (tile, k, name)] = (lambda img=img, tile=tile, nums=nums, out=out:
                                                                      api.score_tile_select(img, tile, nums, DEN, out=out))
                cands["score_tiles_%d_rule_%s" % (tile, name)] = (lambda img=img, tile=tile, rule_out=rule_out:
                                                                  api.score_tiles(img, tile, CAP, planes=RULE, out=rule_out))
            cands["host_%d_1_error_scores" % tile] = (lambda tile=tile: host_quantile(imgs["error_scores"], tile, 19, DEN))
            slow.add("host_%d_1_error_scores" % tile)
        for name, img in imgs.items():
            cands["score_select_1_%s" % name] = (lambda img=img: api.score_select(img, [ref.rank_of(px, 19, DEN)], workspace=ws, result=result))
        # the gate: on the 19/20 plane of the error scores
        grid = api.tile_grid(H, W, GATE_TILE)
        plane = api.score_tile_select(imgs["error_scores"], GATE_TILE, [19], DEN, fields=("value",))["value"][0]
        threshold = float(np.median(plane.cpu().numpy()))
        d_open = torch.empty(grid, dtype=torch.int32, device=dev)
        gate_result = torch.zeros(4, dtype=torch.int64, device=dev)
        counts = torch.randint(0, 64, (H, W), device=dev, generator=gen, dtype=torch.int32)
        gate_imgs = [imgs["error_scores"], counts]
        gate_outs = [torch.empty_like(t) for t in gate_imgs]
        for k in (1, 2):
            cands["gate_tiles_%d_%d_error_scores" % (GATE_TILE, k)] = (lambda k=k: api.gate_tiles(H, W, GATE_TILE, plane, threshold, open=d_open,
                                                                                                   images=gate_imgs[:k], out=gate_outs[:k], result=gate_result))
        # every timed tile_select and gate_tiles configuration against the restatement, before anything is timed
        want = {}
        for tile in ref.TILES:
            for name, img in imgs.items():
                print("restating %d x %d, tile %d, %s" % (W, H, tile, name), file=sys.stderr, flush=True)
                want[(tile, name)] = ref.tile_select_ref(img.cpu().numpy(), tile, RANKS[4], DEN)
        for key, fn in cands.items():
            if key.startswith("tile_select"):
                _, _, tile, k, name = key.split("_", 4)
                got = api.read_tile_quantiles(fn())
                w = want[(int(tile), name)]
                w = w if int(k) == 4 else {f: [w[f][2]] for f in ref.FIELDS}
                if not same(got, w, int(k)):
                    sys.exit("time_score_tile_select.py: %s differs from the restatement at %d x %d" % (key, W, H))
            elif key.startswith("host"):
                tile = int(key.split("_")[1])
                if not np.array_equal(fn().view(np.uint32), want[(tile, "error_scores")]["value"][2].view(np.uint32)):
                    sys.exit("time_score_tile_select.py: %s differs from the restatement at %d x %d" % (key, W, H))
            elif key.startswith("gate_tiles"):
                k = int(key.split("_")[3])
                o, _, res, gated = ref.gate_ref(H, W, GATE_TILE, plane.cpu().numpy(), threshold, None, [t.cpu().numpy() for t in gate_imgs[:k]])
                got_open, got_imgs, got_res = fn()
                ok = api.read_gate_result(got_res) == res and np.array_equal(got_open.cpu().numpy(), o)
                ok = ok and all(np.array_equal(g.cpu().numpy().view(np.uint32), w) for g, w in zip(got_imgs, gated))
                if not ok:
                    sys.exit("time_score_tile_select.py: %s differs from the restatement at %d x %d" % (key, W, H))
                if not 0 < res["n_open"] < res["n_tiles"]:
                    sys.exit("time_score_tile_select.py: %s: the gate leaves %d of %d tiles open, nothing to time" % (key, res["n_open"], res["n_tiles"]))
        runs = {name: [] for name in cands}
        for r in range(a.rounds):                    # alternating: every round times every candidate once
            for name, fn in cands.items():
                if name in slow:
                    runs[name].append(timed(fn, max(a.iters // 5, 1), 2 if r == 0 else 1))
                else:
                    runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
        mean = {name: sum(v) / len(v) for name, v in runs.items()}
        spread = {name: max(v) - min(v) for name, v in runs.items()}
        for key in cands:
            ms = mean[key]
            floor_ms = (8 * int(key.split("_")[3]) if key.startswith("gate_tiles") else 4) * px / bw * 1e3
            line = {"kernel": key, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[key]],
                    "spread_ms": round(spread[key], 4), "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(ms / floor_ms, 2)}
            if key in slow:
                line["calls_per_run"] = max(a.iters // 5, 1)
            if key.startswith("tile_select"):
                _, _, tile, k, name = key.split("_", 4)
                ty, tx = api.tile_grid(H, W, int(tile))
                line.update({"launches": 1, "tiles": ty * tx, "ranks": int(k), "ns_per_tile": round(ms * 1e6 / (ty * tx), 1),
                             "ratio_to_score_tiles_rule": round(ms / mean["score_tiles_%s_rule_%s" % (tile, name)], 2),
                             "ratio_to_score_select": round(ms / mean["score_select_1_%s" % name], 2), "equals_the_restatement": True})
                if name == "error_scores" and int(k) == 1:
                    line["ratio_to_host"] = round(ms / mean["host_%s_1_error_scores" % tile], 4)
            if key.startswith("gate_tiles"):
                line.update({"launches": 2, "images": int(key.split("_")[3]), "equals_the_restatement": True})
            lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
