"""A/B of the accumulation's type-fused walk (statmc_debug_accumulate_fused) at the headline shape: 1920 x 1080, 256 samples per
pixel and launch, the 11-channel set, samples and moments from statmc_malloc_placed, the sample stream of synthetic.Scene generated
as bench.py generates it (--samples uniform: torch.rand in every channel -- the per-type launch is about 3 % slower on those than
on the scene's, the fused one is not: DESIGN.md 4.1).  Fused and per-type launches alternate within ONE process, pair after pair:

  back_to_back  the accumulation launch alone, `--launches` of them between two events
  step          the accumulation (with the pre-pass epilogue) and the window filter behind it, as in bench.py's step, each between
                its own events: median over `--steps` steps, accumulation and filter reported apart

and one JSON line goes to stdout and is appended to --out (default profiles/accumulate_fused.jsonl): per variant the times of
every pair, their median and spread (max - min over the pairs), and the verdict by the project's rule -- the fused walk counts as
a gain when its accumulation time in the step is below the per-type one in EVERY pair and the median difference is at least
three times the larger within-variant spread.

    python tools/time_accumulate_fused.py [--pairs 6] [--ring-depth 3 --vgprs N --agprs N --scratch 0] [--lib PATH]

--ring-depth / --vgprs / --agprs / --scratch describe the build under test (the ring depth is a compile-time constant,
STATMC_ACC_FUSED_D; the register figures are -Rpass-analysis=kernel-resource-usage's for accumulate_fused_kernel<2, 2, D>) and are
recorded as given.  --lib: another build of the library (a ring-depth variant)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from statmc_amd import api, build, film, synthetic  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--channels", type=int, default=11, choices=(9, 11))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10, help="accumulation launches per back-to-back timing")
    ap.add_argument("--steps", type=int, default=10, help="steps per in-the-step timing")
    ap.add_argument("--unplaced", action="store_true", help="buffers from torch's allocator")
    ap.add_argument("--samples", default="scene", choices=("scene", "uniform"),
                    help="scene: synthetic.Scene's stream, generated as bench.py generates it (default); uniform: torch.rand in every channel")
    ap.add_argument("--ring-depth", type=int, default=3)
    ap.add_argument("--vgprs", type=int, default=None)
    ap.add_argument("--agprs", type=int, default=None)
    ap.add_argument("--scratch", type=int, default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--box", default=None, help="a name for the machine, recorded as given")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_fused.jsonl"))
    a = ap.parse_args()
    if a.pairs < 5:
        ap.error("at least five alternating pairs")
    if a.lib:
        build.SO = os.path.abspath(a.lib)
    dev = torch.device("cuda:0")
    api.setup(0)
    W, H, S = a.width, a.height, a.spp
    types = synthetic.FEATURES if a.channels == 11 else synthetic.FEATURES[:3]
    placed = not a.unplaced
    g = torch.Generator(device=dev).manual_seed(1)
    smp = {}
    for t in types:
        shape = (S, H, W, synthetic.CHANNELS[t])
        smp[t] = api.empty_placed(shape, torch.float32, dev, api.MEM_STREAM) if placed else torch.empty(shape, dtype=torch.float32, device=dev)
    scene = synthetic.Scene(W, H, n_regions=12, seed=1, device=dev) if a.samples == "scene" else None
    for s0 in range(0, S, 32):
        n = min(32, S - s0)
        part = scene.samples(n, seed=1000 + s0, features=types) if scene is not None else \
            {t: torch.rand((n,) + tuple(smp[t].shape[1:]), device=dev, generator=g) for t in types}
        for t in types:
            smp[t][s0:s0 + n] = part[t]
        del part
    fs = film.FilmStats(W, H, dev, types=types, placed=placed, fused_prepass=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def back_to_back(mode):
        api.accumulate_fused(mode)
        fs.accumulate(smp)
        ran = api.last_accumulate_fused()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(a.launches):
            fs.accumulate(smp)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.launches, ran

    def step(mode):
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

    names = {1: "fused", -1: "per_type"}
    runs = {n: {"back_to_back_ms": [], "step_accumulate_ms": [], "step_filter_ms": []} for n in names.values()}
    ran_fused = {}
    try:
        for mode in (1, -1):            # warm-up of both variants
            back_to_back(mode)
            step(mode)
        for _ in range(a.pairs):
            for mode in (1, -1):
                ms, ran = back_to_back(mode)
                ran_fused[names[mode]] = ran
                acc, flt = step(mode)
                r = runs[names[mode]]
                r["back_to_back_ms"].append(round(ms, 4))
                r["step_accumulate_ms"].append(round(acc, 4))
                r["step_filter_ms"].append(round(flt, 4))
    finally:
        api.accumulate_fused(0)
    if ran_fused != {"fused": 1, "per_type": 0}:
        raise SystemExit("the switch did not choose the kernels: %s" % ran_fused)
    acc_bytes = sum(synthetic.CHANNELS[t] * 4 * S + (2 * 4 + (10 if t == "radiance" else 2) * 4 * synthetic.CHANNELS[t]) for t in types) + 24
    summary = {}
    for n, r in runs.items():
        summary[n] = dict(r)
        for k in list(r):
            summary[n][k.replace("_ms", "_median_ms")] = round(statistics.median(r[k]), 4)
            summary[n][k.replace("_ms", "_spread_ms")] = round(max(r[k]) - min(r[k]), 4)
        summary[n]["step_accumulate_frac_hbm"] = round(acc_bytes * W * H / (summary[n]["step_accumulate_median_ms"] * 1e-3) / PEAK, 4)
    f, p = runs["fused"]["step_accumulate_ms"], runs["per_type"]["step_accumulate_ms"]
    diff = statistics.median(y - x for x, y in zip(f, p))
    spread = max(summary["fused"]["step_accumulate_spread_ms"], summary["per_type"]["step_accumulate_spread_ms"])
    line = {"tool": "time_accumulate_fused", "film": "%dx%d" % (W, H), "spp": S, "channels": a.channels, "placed": placed, "samples": a.samples,
            "device": torch.cuda.get_device_name(0), "box": a.box, "pid": os.getpid(), "pairs": a.pairs,
            "ring_depth": a.ring_depth, "lds_bytes_per_workgroup": 4 * a.ring_depth * (768 * (3 if a.channels >= 9 else 1) + 256 * (a.channels - 9)) * 4,
            "vgprs": a.vgprs, "agprs": a.agprs, "scratch_bytes": a.scratch, "accumulate_bytes_per_px": acc_bytes,
            "fused": summary["fused"], "per_type": summary["per_type"],
            "step_accumulate_median_gain_ms": round(diff, 4), "larger_spread_ms": round(spread, 4),
            "fused_below_in_every_pair": all(x < y for x, y in zip(f, p)),
            "gain_by_the_rule": bool(all(x < y for x, y in zip(f, p)) and diff >= 3 * spread)}
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
