"""Times statmc_accumulate_records_split -- a pixel's long run split over the 64 lanes of a wave -- against
statmc_accumulate_records (the yardstick) on the same records, at 1920 x 1080 with the five stat types of film.STAT_TYPES
(11 channels), moments and samples from statmc_malloc_placed.  One process per record set:

    python tools/time_accumulate_records_split.py --set a|c|d [--width 1920 --height 1080 --iters 50 --warmup 10]

  a  16 records for every pixel; the records of sample s visit the pixels in a shuffled order of their own.
     No pixel is above any threshold: what the split entry costs here is its check alone.
  c  sparse: 5 % of the pixels at 256 records each, shuffled the same way (4.1c).  Split at split_above = 64 only.
  d  heavy-tailed: one record on every pixel plus 16 pixels with 65 536 records each, all shuffled.

In the same process the sequential entry and the split entry at split_above = 64, 256, 1024, 4096 are each timed five times
(hipEvent, `iters` calls after `warmup`, moments zeroed before every series; mean and spread = max - min), as the whole call and
as the fold alone over the index a grouping-only call left (statmc_debug_accumulate_records_phases); the grouping alone is
timed too.  One JSON line per set.  `faster` / `not_slower` compare the call times with the project's margin of 3 x the larger
of the two spreads.

Before anything is timed every threshold's result from zeroed moments is checked: the pixels up to the threshold must hold the
sequential entry's bits, and a sample of the pixels above it the bits of the DEFINITION (include/statmc.h), rebuilt from existing
entries on a film of just those pixels: statmc_accumulate_records per chunk set, statmc_combine_statistics per tree edge."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402

TYPES = ("radiance", "normal", "albedo", "depth", "materialid")
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
THRESHOLDS = (64, 256, 1024, 4096)
LANES = api.RECORDS_SPLIT_LANES
MARGIN = 3.0
CHECKED_PIXELS = 4


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


def placed_copy(t, dev):
    out = api.empty_placed(tuple(t.shape), t.dtype, dev, api.MEM_STREAM)
    out.copy_(t)
    return out


def make_pixels(which, npx, dev, gen):
    """the record set's pixel array, int32 [n_records]"""
    if which == "d":
        heavy = torch.randperm(npx, device=dev, generator=gen)[:16]
        px = torch.cat([torch.arange(npx, device=dev), heavy.repeat_interleave(65536)])
        return px[torch.randperm(px.numel(), device=dev, generator=gen)].to(torch.int32).contiguous()
    S = 16 if which == "a" else 256
    subset = torch.arange(npx, device=dev) if which == "a" else torch.randperm(npx, device=dev, generator=gen)[:npx // 20]
    idx = torch.stack([subset[torch.randperm(subset.numel(), device=dev, generator=gen)] for _ in range(S)])
    return idx.to(torch.int32).reshape(-1).contiguous()


def definition_bits(W_small, pixels_small, samples_small, ch, cfg, dev):
    """The definition on a film of W_small x 1 pixels, every one of them split, from zeroed moments: 64 sets of images, chunk j
    of every pixel's run into set j by statmc_accumulate_records (the other records set to -1), the tree of
    statmc_combine_statistics.  Returns set 0's images."""
    n = pixels_small.numel()
    slot = torch.full((n,), -1, dtype=torch.int64, device=dev)
    for p in range(W_small):
        idx = (pixels_small == p).nonzero().reshape(-1)              # ascending record index
        L = -(-idx.numel() // LANES)
        slot[idx] = torch.arange(idx.numel(), device=dev) // L
    sets = [{t: film.new_state(1, W_small, ch[t], dev, transform=cfg[t]["transform"]) for t in TYPES} for _ in range(LANES)]
    dead = torch.full_like(pixels_small, -1)
    for j in range(LANES):
        px = torch.where(slot == j, pixels_small, dead).contiguous()
        api.accumulate_records(W_small, 1, [api.make_stat_type_records(samples_small[t], ch[t], sets[j][t], cfg[t]["transform"], cfg[t]["max_moment"])
                                            for t in TYPES], px)
    stride = 1
    while stride < LANES:
        for j in range(0, LANES, 2 * stride):
            api.combine_statistics(W_small, 1, [api.make_combine_entry(sets[j][t], sets[j + stride][t], ch[t], cfg[t]["max_moment"]) for t in TYPES])
        stride *= 2
    torch.cuda.synchronize()
    return [sets[0][t][k].reshape(W_small, -1) for t in TYPES for k in FIELDS if sets[0][t].get(k) is not None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("a", "c", "d"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    dev = torch.device("cuda:0")
    api.setup(0)
    cfg = film.STAT_TYPES
    ch = {t: cfg[t]["channels"] for t in TYPES}
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = api.current_stream_handle()

    pixels = make_pixels(a.set, npx, dev, gen)
    n_rec = pixels.numel()
    counts = torch.bincount(pixels.to(torch.int64), minlength=npx)
    samples = {}
    for t in TYPES:          # positive values (the radiance type takes a square root); u^2 keeps some of them small
        u = torch.rand(n_rec, ch[t], device=dev, generator=gen)
        samples[t] = placed_copy(u * u + 0.01, dev)
        del u
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    rec_types = [api.make_stat_type_records(samples[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    def call(split_above):
        return lambda: api.accumulate_records(W, H, rec_types, pixels, stream=stream, split_above=split_above)

    def phases(p):
        api.check(api.load().statmc_debug_accumulate_records_phases(p))

    def images():
        return [fs.state[t][k].reshape(npx, -1) for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    # ---- the results, before anything is timed
    fs.reset()
    call(None)()
    torch.cuda.synchronize()
    sequential = [img.clone() for img in images()]
    same_bits = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    checks = {}
    for k in THRESHOLDS:
        fs.reset()
        call(k)()
        torch.cuda.synchronize()
        got = images()
        long_px = counts > k
        short_ok = all(same_bits(g[~long_px], s[~long_px]) for g, s in zip(got, sequential))
        sample = long_px.nonzero().reshape(-1)[:CHECKED_PIXELS]
        entry = {"long_pixels": int(long_px.sum()), "short_pixels_equal_sequential": bool(short_ok), "long_pixels_checked": int(sample.numel())}
        if sample.numel():
            member = torch.zeros(npx, dtype=torch.bool, device=dev)
            member[sample] = True
            rec_idx = member[pixels.to(torch.int64)].nonzero().reshape(-1)          # ascending record index
            remap = torch.full((npx,), -1, dtype=torch.int32, device=dev)
            remap[sample] = torch.arange(sample.numel(), dtype=torch.int32, device=dev)
            px_small = remap[pixels[rec_idx].to(torch.int64)].contiguous()
            smp_small = {t: samples[t][rec_idx].contiguous() for t in TYPES}
            want = definition_bits(int(sample.numel()), px_small, smp_small, ch, cfg, dev)
            entry["long_pixels_equal_definition"] = bool(all(same_bits(g[sample], w) for g, w in zip(got, want)))
            entry["long_pixels_differ_from_sequential_in_bits"] = bool(any(not same_bits(g[sample], s[sample]) for g, s in zip(got, sequential)))
        checks[str(k)] = entry
    del sequential

    # ---- timings
    def series(fn):
        runs = []
        for _ in range(5):
            fs.reset()
            runs.append(timed(fn, a.iters, a.warmup))
        return {"ms": round(sum(runs) / len(runs), 4), "spread_ms": round(max(runs) - min(runs), 4), "runs_ms": [round(v, 4) for v in runs]}

    def measure(split_above):
        fn = call(split_above)
        out = {"call": series(fn)}
        phases(1)
        out["grouping"] = series(fn)
        phases(2)                                        # over the index the grouping-only calls left in the workspace
        out["fold"] = series(fn)
        phases(3)
        return out

    seq = measure(None)
    split = {str(k): measure(k) for k in THRESHOLDS}
    for k, m in split.items():
        margin = MARGIN * max(m["call"]["spread_ms"], seq["call"]["spread_ms"])
        m["call_over_sequential"] = round(m["call"]["ms"] / seq["call"]["ms"], 4)
        m["fold_over_sequential"] = round(m["fold"]["ms"] / seq["fold"]["ms"], 4)
        m["margin_ms"] = round(margin, 4)
        m["faster"] = bool(m["call"]["ms"] < seq["call"]["ms"] - margin)
        m["not_slower"] = bool(m["call"]["ms"] <= seq["call"]["ms"] + margin)
    print(json.dumps({
        "set": a.set, "width": W, "height": H, "records": n_rec, "touched_pixels": int((counts > 0).sum()), "longest_run": int(counts.max()),
        "channels": sum(ch.values()), "iters": a.iters, "warmup": a.warmup, "placed": api.placement_info()["active"] == 1,
        "checks": checks, "sequential": seq, "split": split,
    }), flush=True)


if __name__ == "__main__":
    main()
