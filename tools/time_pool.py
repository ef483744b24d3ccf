"""Times statmc_pool_statistics at 1920 x 1080 on the 11-channel FilmStats set plus "film", for k = 2, 4 and 8, against
statmc_combine_statistics over the same fine film -- the closest existing launch: one merge per pixel, three times the fine bytes,
HBM-bound -- all in one process, the candidates alternating over several rounds.  One JSON line per kernel: milliseconds per call
(hipEvent timing after warm-up; mean, and the runs), the algorithmic bytes computed from the shapes, TB/s and the time relative to
the combine call.

    python tools/time_pool.py [--width 1920 --height 1080 --iters 200 --warmup 20 --rounds 5] [--out profiles/pool_statistics.jsonl]

Algorithmic bytes.  pool: B_fine + B_coarse -- every pooled plane and every owned count image read once at the fine size and
written once at the coarse size, the epilogue's mean-corr / discriminator written at the coarse size.  combine: both sides of every
plane read and the dst side written, 3 B_fine (+ the epilogue's two images).
Merges per fine pixel of the lane mapping (statmc_pool.hip): a lane merges its 2 x 2 sub-block itself (3 merges for 4 pixels) and
merge_lanes<k * k / 4> runs log2(k * k / 4) more per lane: 0.75, 1.25, 1.75 for k = 2, 4, 8; the combine call runs 1."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402

TYPES = ("radiance", "normal", "albedo", "depth", "materialid")


def fill(fs, gen):
    for t in fs.types:
        for key, v in fs.state[t].items():
            if v is None:
                continue
            if key == "n":
                v.copy_(torch.randint(1, 64, v.shape, dtype=torch.int32, device=v.device, generator=gen))
            else:
                v.copy_(torch.rand(v.shape, device=v.device, generator=gen))
    fs.film.copy_(torch.rand(fs.film.shape, device=fs.film.device, generator=gen))


def state_bytes(fs, epilogue):
    """bytes of one film of fs's size: the planes and counts a pool or combine entry moves (+ mean-corr / discriminator)"""
    px = fs.width * fs.height
    total = px * 3 * 4                                       # "film"
    for t in fs.types:
        cfg = film.STAT_TYPES[t]
        planes = cfg["max_moment"] + (2 if cfg["transform"] else 0)
        total += px * (4 + planes * cfg["channels"] * 4)
    return total, (2 * px * 3 * 4 if epilogue else 0)


def pool_entries(fine, coarse):
    es = []
    for t in fine.types:
        cfg = film.STAT_TYPES[t]
        es.append(api.make_pool_entry(coarse.state[t], fine.state[t], cfg["channels"], cfg["max_moment"],
                                      prepass_into=(coarse.mean_corr, coarse.disc) if t == "radiance" else None))
    es.append(api.make_pool_entry({"mean": coarse.film}, {"mean": fine.film}, 3, 1, count_of=fine.types.index("radiance")))
    return es


def combine_entries(a, b):
    es = []
    for t in a.types:
        cfg = film.STAT_TYPES[t]
        es.append(api.make_combine_entry(a.state[t], b.state[t], cfg["channels"], cfg["max_moment"],
                                         prepass_into=(a.mean_corr, a.disc) if t == "radiance" else None))
    es.append(api.make_combine_entry({"mean": a.film}, {"mean": b.film}, 3, 1, count_of=a.types.index("radiance")))
    return es


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_pool.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    W, H = a.width, a.height
    fine, other = film.FilmStats(W, H, dev, types=TYPES), film.FilmStats(W, H, dev, types=TYPES)
    fill(fine, gen)
    fill(other, gen)
    b_fine, pre_fine = state_bytes(fine, True)
    cands = {}
    ces = combine_entries(other, fine)           # `other` accumulates: counts stay far below 2^24 over the timed calls
    cands["combine"] = (lambda: api.combine_statistics(W, H, ces), 3 * b_fine + pre_fine, 1.0)
    keep = []
    for k in (2, 4, 8):
        wc, hc = api.pooled_size(W, H, k)
        coarse = film.FilmStats(wc, hc, dev, types=TYPES)
        b_coarse, pre_coarse = state_bytes(coarse, True)
        es = pool_entries(fine, coarse)
        keep.append((coarse, es))
        cands["pool_k%d" % k] = ((lambda es=es, k=k: api.pool_statistics(W, H, k, es)), b_fine + b_coarse + pre_coarse,
                                 0.75 + math.log2(k * k // 4) / 4)
    runs = {name: [] for name in cands}
    for r in range(a.rounds):                    # alternating: every round times every candidate once
        for name, (fn, _, _) in cands.items():
            if name == "combine":
                for t in other.types:
                    other.state[t]["n"].fill_(1)
            runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
    base = sum(runs["combine"]) / len(runs["combine"])
    lines = []
    for name, (_, nbytes, merges) in cands.items():
        ms = sum(runs[name]) / len(runs[name])
        lines.append(json.dumps({"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                                 "spread_ms": round(max(runs[name]) - min(runs[name]), 4), "bytes": nbytes,
                                 "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3), "merges_per_fine_pixel": merges,
                                 "ratio_to_combine": round(ms / base, 4)}))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
