"""The accumulation fed IEEE-half sample arenas (statmc_accumulate_formats) against the fp32 launch it replaces (statmc_accumulate,
the shipped dispatch), on the same values: the sample stream of synthetic.Scene generated as bench.py generates it, rounded to
half (radiance clamped to the largest finite half first, as a renderer that keeps radiance in half must), kept as that arena and
as its widened fp32 copy.  One process, samples and moments from statmc_malloc_placed.  fp32 and 16-bit launches alternate, pair
after pair:

  back_to_back  the accumulation launch alone, `--launches` of them between two events
  step          the accumulation (with the pre-pass epilogue) and the window filter behind it, as in bench.py's step, each between
                its own events: median over `--steps` steps, accumulation and filter reported apart

One JSON line per mix goes to stdout and is appended to --out (default profiles/accumulate_half.jsonl): per variant the times of
every pair, their median and spread (max - min over the pairs), the bytes per pixel by the model (sum 2 C16 + sum 4 C32) S + 224
(+ 24 for the pre-pass epilogue these launches carry), the fraction of 8 TB/s they give, and the verdict by the project's rule -- the 16-bit
launch counts as a gain when its accumulation time in the step is below the fp32 one in EVERY pair and the median difference is
at least three times the larger within-variant spread.

    python tools/time_accumulate_half.py [--width 1920 --height 1080 --spp 256] [--mix both|all_half|features_half] [--half-fused 0|1|-1]

--half-fused: statmc_debug_accumulate_fused for the 16-bit launches only (0: the shipped dispatch; -1: the per-type 16-bit kernel;
the fp32 launches always run the shipped dispatch)."""
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
MIXES = {"all_half": lambda t: True, "features_half": lambda t: t != "radiance"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--channels", type=int, default=11, choices=(9, 11))
    ap.add_argument("--mix", default="both", choices=("both",) + tuple(MIXES))
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10, help="accumulation launches per back-to-back timing")
    ap.add_argument("--steps", type=int, default=10, help="steps per in-the-step timing")
    ap.add_argument("--half-fused", type=int, default=0, choices=(-1, 0, 1))
    ap.add_argument("--box", default=None, help="a name for the machine, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_half.jsonl"))
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("at least five alternating pairs")
    dev = torch.device("cuda:0")
    api.setup(0)
    W, H, S = a.width, a.height, a.spp
    types = synthetic.FEATURES if a.channels == 11 else synthetic.FEATURES[:3]
    mixes = list(MIXES) if a.mix == "both" else [a.mix]
    need_half = [t for t in types if any(MIXES[m](t) for m in mixes)]
    wide, half = {}, {}
    for t in types:
        shape = (S, H, W, synthetic.CHANNELS[t])
        wide[t] = api.empty_placed(shape, torch.float32, dev, api.MEM_STREAM)
        if t in need_half:
            half[t] = api.empty_placed(shape, torch.float16, dev, api.MEM_STREAM)
    scene = synthetic.Scene(W, H, n_regions=12, seed=1, device=dev)
    for s0 in range(0, S, 32):
        n = min(32, S - s0)
        part = scene.samples(n, seed=1000 + s0, features=types)
        for t in types:
            h = part[t].clamp(-HALF_MAX, HALF_MAX).half()
            wide[t][s0:s0 + n] = h.float()              # the same values in both variants
            if t in half:
                half[t][s0:s0 + n] = h
        del part
    fs = film.FilmStats(W, H, dev, types=types, placed=True, fused_prepass=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def back_to_back(smp, mode):
        api.accumulate_fused(mode)
        fs.accumulate(smp)
        ran = (api.last_accumulate_loader(), api.last_accumulate_fused(), int(api.load().statmc_debug_last_accumulate_grid()))
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(a.launches):
            fs.accumulate(smp)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches, ran

    def step(smp, mode):
        api.accumulate_fused(mode)
        for _ in range(2):
            fs.accumulate(smp)
            fs.window_filter()
        marks = []
        for _ in range(a.steps):
            e = [ev(), ev(), ev()]
            e[0].record()
            fs.accumulate(smp)
            e[1].record()
            fs.window_filter()
            e[2].record()
            marks.append(e)
        torch.cuda.synchronize()
        return (statistics.median(e[0].elapsed_time(e[1]) for e in marks), statistics.median(e[1].elapsed_time(e[2]) for e in marks))

    state_bytes = sum(2 * 4 + (10 if t == "radiance" else 2) * 4 * synthetic.CHANNELS[t] for t in types) + 24
    for mix in mixes:
        given = {t: (half[t] if MIXES[mix](t) else wide[t]) for t in types}
        variants = {"fp32": (wide, 0), "half": (given, a.half_fused)}
        runs = {n: {"back_to_back_ms": [], "step_accumulate_ms": [], "step_filter_ms": []} for n in variants}
        ran = {}
        try:
            for smp, mode in variants.values():            # warm-up of both variants
                back_to_back(smp, mode)
                step(smp, mode)
            for _ in range(a.pairs):
                for name, (smp, mode) in variants.items():
                    ms, ran[name] = back_to_back(smp, mode)
                    acc, flt = step(smp, mode)
                    r = runs[name]
                    r["back_to_back_ms"].append(round(ms, 4))
                    r["step_accumulate_ms"].append(round(acc, 4))
                    r["step_filter_ms"].append(round(flt, 4))
        finally:
            api.accumulate_fused(0)
        if ran["fp32"][0] != 0 or ran["half"][0] != 1:
            raise SystemExit("the launches did not take the loaders they were meant to: %s" % ran)
        bytes_px = {"fp32": sum(4 * synthetic.CHANNELS[t] for t in types) * S + state_bytes,
                    "half": sum((2 if MIXES[mix](t) else 4) * synthetic.CHANNELS[t] for t in types) * S + state_bytes}
        summary = {}
        for n, r in runs.items():
            summary[n] = dict(r)
            for k in list(r):
                summary[n][k.replace("_ms", "_median_ms")] = round(statistics.median(r[k]), 4)
                summary[n][k.replace("_ms", "_spread_ms")] = round(max(r[k]) - min(r[k]), 4)
            summary[n]["bytes_per_px"] = bytes_px[n]
            summary[n]["step_accumulate_frac_hbm"] = round(bytes_px[n] * W * H / (summary[n]["step_accumulate_median_ms"] * 1e-3) / PEAK, 4)
            summary[n]["back_to_back_frac_hbm"] = round(bytes_px[n] * W * H / (summary[n]["back_to_back_median_ms"] * 1e-3) / PEAK, 4)
            summary[n]["loader_fused_grid"] = list(ran[n])
        h, f = runs["half"]["step_accumulate_ms"], runs["fp32"]["step_accumulate_ms"]
        diff = statistics.median(y - x for x, y in zip(h, f))
        spread = max(summary["half"]["step_accumulate_spread_ms"], summary["fp32"]["step_accumulate_spread_ms"])
        line = {"tool": "time_accumulate_half", "film": "%dx%d" % (W, H), "spp": S, "channels": a.channels, "mix": mix, "placed": True,
                "samples": "scene", "half_fused_switch": a.half_fused, "device": torch.cuda.get_device_name(0), "box": a.box,
                "pid": os.getpid(), "pairs": a.pairs, "fp32": summary["fp32"], "half": summary["half"],
                "bytes_ratio": round(bytes_px["half"] / bytes_px["fp32"], 4),
                "time_ratio": round(summary["half"]["step_accumulate_median_ms"] / summary["fp32"]["step_accumulate_median_ms"], 4),
                "step_accumulate_median_gain_ms": round(diff, 4), "larger_spread_ms": round(spread, 4),
                "half_below_in_every_pair": all(x < y for x, y in zip(h, f)),
                "gain_by_the_rule": bool(all(x < y for x, y in zip(h, f)) and diff >= 3 * spread)}
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
