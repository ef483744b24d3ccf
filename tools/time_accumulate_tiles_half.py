"""The tile-fed accumulation given IEEE-half arenas (statmc_accumulate_tiles_formats) against the fp32 tile launch it replaces
(statmc_accumulate_tiles, the shipped dispatch), on the same values: the sample stream of synthetic.Scene rounded to half
(radiance clamped to the largest finite half first), cut into 16 x 16 tile blocks [tile][S][h][16][C], kept as that arena and as
its widened fp32 copy.  One process, arenas and moments from statmc_malloc_placed.  The variants alternate, round after round:

  fp32        statmc_accumulate_tiles on the widened arenas
  half        the half launch with statmc_debug_accumulate_dma 1: the launch's RGB rows, fp32 and half, by LDS-DMA
  half_reg    the half launch with statmc_debug_accumulate_dma 0: every row by register loads

Each timing is `--launches` launches between two events.  One JSON line per mix goes to stdout and is appended to --out (default
profiles/accumulate_tiles_half.jsonl): per variant the time of every round, the median and the spread (max - min over the
rounds), the bytes per pixel by the model (sum 2 C16 + sum 4 C32) S + 200, and per pair of variants the verdict by the project's
rule -- the one with the smaller median counts as a gain over the other when it is below it in EVERY round and the median
difference is at least three times the larger within-variant spread.

    python tools/time_accumulate_tiles_half.py [--width 1920 --height 1080 --spp 64] [--mix both|all_half|features_half]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from statmc_amd import api, film, synthetic  # noqa: E402

PEAK = 8.0e12
HALF_MAX = 65504.0
T = 16
MIXES = {"all_half": lambda t: True, "features_half": lambda t: t != "radiance"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64, help="samples per tile and launch")
    ap.add_argument("--channels", type=int, default=11, choices=(9, 11))
    ap.add_argument("--mix", default="both", choices=("both",) + tuple(MIXES))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--box", default=None, help="a name for the machine, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_tiles_half.jsonl"))
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("at least five alternating rounds")
    if a.width % T:
        ap.error("the film's width must be a multiple of %d" % T)
    dev = torch.device("cuda:0")
    api.setup(0)
    W, H, S = a.width, a.height, a.spp
    types = synthetic.FEATURES if a.channels == 11 else synthetic.FEATURES[:3]
    mixes = list(MIXES) if a.mix == "both" else [a.mix]
    bands = [(y, min(y + T, H)) for y in range(0, H, T)]
    bounds, offsets, off = [], [], 0
    for y0, y1 in bands:
        for x0 in range(0, W, T):
            bounds.append((x0, y0, x0 + T, y1))
            offsets.append(off)
            off += S * (y1 - y0) * T
    total = off
    wide, half = {}, {}
    for t in types:
        c = synthetic.CHANNELS[t]
        wide[t] = api.empty_placed((total * c,), torch.float32, dev, api.MEM_STREAM)
        if any(MIXES[m](t) for m in mixes):
            half[t] = api.empty_placed((total * c,), torch.float16, dev, api.MEM_STREAM)
    scene = synthetic.Scene(W, H, n_regions=12, seed=1, device=dev)
    band_at = [offsets[i * (W // T)] for i in range(len(bands))]
    for s0 in range(0, S, 16):
        n = min(16, S - s0)
        part = scene.samples(n, seed=1000 + s0, features=types)
        for t in types:
            c = synthetic.CHANNELS[t]
            h16 = part[t].clamp(-HALF_MAX, HALF_MAX).half()                       # [n, H, W, c]
            for (y0, y1), at in zip(bands, band_at):
                hb = y1 - y0
                blk = h16[:, y0:y1].reshape(n, hb, W // T, T, c).permute(2, 0, 1, 3, 4)       # [tile, n, hb, T, c]
                for dst, src in ((wide[t], blk.float()), (half.get(t), blk)):
                    if dst is not None:
                        dst[at * c:(at + (W // T) * S * hb * T) * c].view(W // T, S, hb, T, c)[:, s0:s0 + n] = src
        del part
    tab = (torch.tensor(bounds, dtype=torch.int32, device=dev), torch.tensor(offsets, dtype=torch.int64, device=dev),
           torch.full((len(bounds),), S, dtype=torch.int32, device=dev))
    state = {t: film.new_state(H, W, synthetic.CHANNELS[t], dev, film.STAT_TYPES[t]["transform"], placed=True) for t in types}

    def stat_types(arenas):
        return [api.make_stat_type_arena(arenas[t], synthetic.CHANNELS[t], state[t], film.STAT_TYPES[t]["transform"],
                                         film.STAT_TYPES[t]["max_moment"]) for t in types]

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(sts, fmts, dma):
        api.accumulate_dma(dma)
        try:
            api.accumulate_tiles(W, H, sts, *tab, sample_formats=fmts)
            torch.cuda.synchronize()
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(a.launches):
                api.accumulate_tiles(W, H, sts, *tab, sample_formats=fmts)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.launches
        finally:
            api.accumulate_dma(1)

    state_bytes = sum(2 * 4 + (10 if t == "radiance" else 2) * 4 * synthetic.CHANNELS[t] for t in types)
    for mix in mixes:
        given = {t: (half[t] if MIXES[mix](t) else wide[t]) for t in types}
        fmts = [api.SAMPLES_F16 if MIXES[mix](t) else api.SAMPLES_F32 for t in types]
        variants = {"fp32": (stat_types(wide), None, 1), "half": (stat_types(given), fmts, 1), "half_reg": (stat_types(given), fmts, 0)}
        runs = {n: [] for n in variants}
        for v in variants.values():                                                # warm-up of every variant
            timed(*v)
        for _ in range(a.rounds):
            for name, v in variants.items():
                runs[name].append(round(timed(*v), 4))
        bytes_px = {n: sum((2 if (v[1] is not None and MIXES[mix](t)) else 4) * synthetic.CHANNELS[t] for t in types) * S + state_bytes
                    for n, v in variants.items()}
        summary = {n: {"ms": r, "median_ms": round(statistics.median(r), 4), "spread_ms": round(max(r) - min(r), 4), "bytes_per_px": bytes_px[n],
                       "frac_hbm": round(bytes_px[n] * W * H / (statistics.median(r) * 1e-3) / PEAK, 4)} for n, r in runs.items()}

        def verdict(x, y):
            fast, slow = (x, y) if summary[x]["median_ms"] <= summary[y]["median_ms"] else (y, x)
            diff = statistics.median(y - x for x, y in zip(runs[fast], runs[slow]))
            spread = max(summary[fast]["spread_ms"], summary[slow]["spread_ms"])
            every = all(x < y for x, y in zip(runs[fast], runs[slow]))
            return {"faster": fast, "slower": slow, "median_gain_ms": round(diff, 4), "larger_spread_ms": round(spread, 4),
                    "below_in_every_round": every, "gain_by_the_rule": bool(every and diff >= 3 * spread)}

        line = {"tool": "time_accumulate_tiles_half", "film": "%dx%d" % (W, H), "samples_per_tile": S, "channels": a.channels, "mix": mix,
                "placed": True, "samples": "scene", "device": torch.cuda.get_device_name(0), "box": a.box,
                "rounds": a.rounds, "launches": a.launches, "variants": summary,
                "half_against_fp32": verdict("half", "fp32"), "ring_against_registers": verdict("half", "half_reg")}
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
