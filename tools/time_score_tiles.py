"""Times statmc_score_tiles at 1920 x 1080 and 3840 x 2160, in one process, against the library's whole-film entries and its float
tile moments:

  score_tiles     tile 8, 16, 32 and 64; all eight planes, and mean + max + n_clipped alone (a tile rule's three); cap 0.05, on
                    random_exponent   every exponent equally likely: a lane's run (statmc_score_tiles.hip) ends at nearly every pixel
                    error_scores      statmc_error_scores of random statistics, 2 to 9 samples per pixel, some below 2 (+inf)
                    constant          one score everywhere: every lane on the same limbs, one run per lane
  score_sum       statmc_score_sum with one cap on the same three images: the same arithmetic for the film as a whole
  tile_moments    statmc_tile_moments at 8 and 16 on the error-score image: float Welford merges, no caps, no classes
  count_above     statmc_score_count_above with one threshold on the random image: one pass over the same bytes
  floor           one read of `score` (4 B/px) at the copy bandwidth measured in the same process (a device-to-device copy of
                  512 MiB: bytes read plus bytes written over its time)

Nothing is reported unless every timed score_tiles configuration equals the restatement in Python integers
(tests/score_tiles_reference.py) bit for bit.  One JSON line per (size, candidate): milliseconds per call (hipEvent timing, 50 calls
after 10, five alternating rounds: every round times every candidate once; mean over the rounds, and the runs), spread = max - min
over the rounds.

    python tools/time_score_tiles.py [--iters 50 --warmup 10 --rounds 5] [--sizes 1920x1080,3840x2160] [--out profiles/score_tiles.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_tiles_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402
from time_score_sum import copy_bandwidth, images, timed  # noqa: E402

CAP = 0.05
RULE = ("mean", "max", "n_clipped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score_tiles.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    bw = copy_bandwidth(dev, 20, 3)
    lines = [json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})]
    for W, H in (tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")):
        px = W * H
        imgs = images(W, H, dev, gen)
        dtypes = {"sum": torch.float64, "sum_sq": torch.float64, "mean": torch.float32, "max": torch.float32,
                  "n_px": torch.int32, "n_zero": torch.int32, "n_infinite": torch.int32, "n_clipped": torch.int32}
        ws = torch.empty(api.score_sum_workspace(), dtype=torch.uint8, device=dev)
        result = torch.zeros(19, dtype=torch.int64, device=dev)
        above = torch.zeros(1, dtype=torch.int64, device=dev)
        cands = {}
        for tile in ref.TILES:
            out = {p: torch.empty(api.tile_grid(H, W, tile), dtype=dtypes[p], device=dev) for p in ref.PLANES}
            for name, img in imgs.items():
                for label, planes in (("all", ref.PLANES), ("rule", RULE)):
                    cands["score_tiles_%d_%s_%s" % (tile, label, name)] = (lambda img=img, tile=tile, planes=planes, out=out:
                                                                           api.score_tiles(img, tile, CAP, planes=planes, out=out))
        for name, img in imgs.items():
            cands["score_sum_1_%s" % name] = (lambda img=img: api.score_sum(img, [CAP], workspace=ws, result=result))
        cands["count_above_1_random_exponent"] = lambda: api.score_count_above(imgs["random_exponent"], [CAP], out=above)
        for tile in (8, 16):
            ty, tx = api.tile_grid(H, W, tile)
            moments = torch.empty((ty, tx, 1, 3), dtype=torch.float32, device=dev)
            cands["tile_moments_%d_error_scores" % tile] = (lambda tile=tile, moments=moments: api.tile_moments(imgs["error_scores"], tile, moments))
        # every timed score_tiles configuration against the restatement, before anything is timed
        want = {}
        for tile in ref.TILES:
            for name, img in imgs.items():
                print("restating %d x %d, tile %d, %s" % (W, H, tile, name), file=sys.stderr, flush=True)
                want[(tile, name)] = ref.tiles_ref(img.cpu().numpy(), tile, CAP)
        for key, fn in cands.items():
            if key.startswith("score_tiles"):
                _, _, tile, label, name = key.split("_", 4)
                planes = ref.PLANES if label == "all" else RULE
                got = api.read_tile_scores(fn())
                if ref.same_bits(got, want[(int(tile), name)], planes):
                    sys.exit("time_score_tiles.py: %s differs from the restatement at %d x %d" % (key, W, H))
        runs = {name: [] for name in cands}
        for r in range(a.rounds):                    # alternating: every round times every candidate once
            for name, fn in cands.items():
                runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
        floor_ms = 4 * px / bw * 1e3
        mean = {name: sum(v) / len(v) for name, v in runs.items()}
        spread = {name: max(v) - min(v) for name, v in runs.items()}
        for key in cands:
            ms = mean[key]
            line = {"kernel": key, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[key]],
                    "spread_ms": round(spread[key], 4), "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(ms / floor_ms, 2)}
            if key.startswith("score_tiles"):
                _, _, tile, label, name = key.split("_", 4)
                ty, tx = api.tile_grid(H, W, int(tile))
                line.update({"launches": 1, "tiles": ty * tx, "ns_per_tile": round(ms * 1e6 / (ty * tx), 1),
                             "ratio_to_score_sum": round(ms / mean["score_sum_1_%s" % name], 2), "equals_the_restatement": True})
                if int(tile) in (8, 16) and name == "error_scores":
                    line["ratio_to_tile_moments"] = round(ms / mean["tile_moments_%s_error_scores" % tile], 2)
            lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
