"""Times statmc_combine_records (and statmc_gather_states) -- the states of listed pixels as (pixel, state) records -- against what a
caller could use instead, at 1920 x 1080 with the five stat types of film.STAT_TYPES (11 channels, 28 dwords of state per pixel,
116 B per record with its pixel index).  One process per set:

    python tools/time_combine_records.py --set a|b|c|d [--out profiles/combine_records.jsonl --iters 50 --warmup 10 --rounds 5]

  a  one record per pixel, in raster order.  Yardstick: the whole-film statmc_combine_statistics of the film the records came from.
  b  one record on 5 % of the pixels, shuffled.  Yardsticks: the whole-film combine; statmc_accumulate_records on the 16 samples per
     record that those states summarise.
  c  four records on a quarter of the pixels, shuffled.  Yardstick: the whole-film combine (one part: for scale).
  d  one record per pixel plus 16 pixels with 4096 records each.  split_above = STATMC_RECORDS_SPLIT_DEFAULT against INT32_MAX.

The records are statmc_gather_states of a source film that holds 16 samples on the listed pixels.  Before anything is timed,
sets a and b check that the records entry leaves the bits of the whole-film combine (`bits_equal`).  Then `rounds` rounds time every
entry alternately in this one process, `iters` calls after `warmup` each (hipEvent timing, the destination zeroed before each
series, so no count passes 2^24); mean over the rounds, spread = max - min.

Per set one JSON line (appended to --out as well): the ms of each entry and the byte model -- (4 + 4 * 28) B per record, 8 B of
sort pair per record, 2 x the state bytes of the touched pixels -- over the call's time as a share of the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402

PEAK = 8.0e12
TYPES = ("radiance", "normal", "albedo", "depth", "materialid")
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
INT32_MAX = 2 ** 31 - 1
SPP = 16


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
    ap.add_argument("--set", choices=("a", "b", "c", "d"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file as well")
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    dev = torch.device("cuda:0")
    api.setup(0)
    cfg = film.STAT_TYPES
    ch = {t: cfg[t]["channels"] for t in TYPES}
    dw = {t: api.state_dwords(ch[t], cfg[t]["max_moment"], cfg[t]["transform"]) for t in TYPES}
    stream = api.current_stream_handle()
    gen = torch.Generator(device=dev).manual_seed(7)

    # ---- the listed pixels, and the source film: SPP samples on each of them
    perm = torch.randperm(npx, device=dev, generator=gen)
    if a.set == "a":
        listed = torch.arange(npx, device=dev)
        pixels = listed
    elif a.set == "b":
        listed = perm[:npx // 20]
        pixels = listed
    elif a.set == "c":
        listed = perm[:npx // 4]
        pixels = listed.repeat(4)[torch.randperm(4 * listed.numel(), device=dev, generator=gen)]
    else:
        listed = torch.arange(npx, device=dev)
        pixels = torch.cat([listed, perm[:16].repeat(4096)])
        pixels = pixels[torch.randperm(pixels.numel(), device=dev, generator=gen)]
    pixels = pixels.to(torch.int32).contiguous()
    n_records, touched = pixels.numel(), listed.numel()
    owners = listed.to(torch.int32).repeat_interleave(SPP).contiguous()           # the samples behind the states, as records
    samples = {t: torch.rand((owners.numel(), ch[t]), device=dev, generator=gen).square_().add_(0.01) for t in TYPES}
    src = film.FilmStats(W, H, dev, types=TYPES)
    dst = film.FilmStats(W, H, dev, types=TYPES)

    def types_of(fs, sample_arrays=None):
        if sample_arrays is None:
            return [api.make_stat_type_record_field(ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]
        return [api.make_stat_type_records(sample_arrays[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    api.accumulate_records(W, H, types_of(src, samples), owners, stream=stream)
    states = api.gather_states(W, H, types_of(src), pixels, stream=stream)
    torch.cuda.synchronize()
    assert int(src.state["radiance"]["n"].sum()) == SPP * touched and all(int(s[:, 0].min()) == SPP for s in states)
    if a.set != "b":
        del samples, owners

    dst_types = types_of(dst)
    dense_entries = [api.make_combine_entry(dst.state[t], src.state[t], ch[t], cfg[t]["max_moment"]) for t in TYPES]
    split = api.RECORDS_SPLIT_DEFAULT if a.set == "d" else INT32_MAX
    gathered = [torch.empty_like(s) for s in states]
    runs = {"combine_records": lambda: api.combine_records(W, H, dst_types, pixels, states, split_above=split, stream=stream),
            "gather_states": lambda: api.gather_states(W, H, types_of(src), pixels, out=gathered, stream=stream),
            "combine_statistics": lambda: api.combine_statistics(W, H, dense_entries, stream=stream)}
    if a.set == "b":
        sample_types = types_of(dst, samples)
        runs["accumulate_records"] = lambda: api.accumulate_records(W, H, sample_types, owners, stream=stream)
    if a.set == "d":
        runs["combine_records_never_split"] = lambda: api.combine_records(W, H, dst_types, pixels, states, split_above=INT32_MAX, stream=stream)

    def images():
        return [dst.state[t][k] for t in TYPES for k in FIELDS if dst.state[t].get(k) is not None]

    # ---- the same bits as the whole-film combine (one record per listed pixel), or the same counts (several)
    dst.reset()
    runs["combine_statistics"]()
    want = [img.clone() for img in images()]
    dst.reset()
    runs["combine_records"]()
    torch.cuda.synchronize()
    if a.set in ("a", "b"):
        equal = all(torch.equal(g.view(torch.int32), img.view(torch.int32)) for g, img in zip(want, images()))
    else:
        equal = int(dst.state["radiance"]["n"].sum()) == SPP * n_records
    del want
    if not equal:
        print(json.dumps({"set": a.set, "bits_equal": False}), flush=True)
        sys.exit(1)

    # ---- timings, alternating
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            dst.reset()
            ms[k].append(timed(fn, a.iters, a.warmup))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    state_bytes = 4 * sum(dw.values())
    record_bytes = 4 + state_bytes
    model_bytes = (record_bytes + 8) * n_records + 2 * state_bytes * touched
    out = {"set": a.set, "width": W, "height": H, "channels": sum(ch.values()), "state_dwords": sum(dw.values()), "record_bytes": record_bytes,
           "n_records": n_records, "touched_pixels": touched, "longest_run": 4097 if a.set == "d" else (4 if a.set == "c" else 1),
           "split_above": split, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds, "bits_equal": True, "model_bytes": model_bytes,
           "combine_records_of_peak": round(model_bytes / (mean["combine_records"] * 1e-3) / PEAK, 4),
           "whole_film_bytes": 3 * state_bytes * npx}
    for k in runs:
        out[k + "_ms"] = round(mean[k], 4)
        out[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
        out[k + "_runs_ms"] = [round(v, 4) for v in ms[k]]
    out["records_over_whole_film"] = round(mean["combine_records"] / mean["combine_statistics"], 3)
    if "accumulate_records" in runs:
        out["records_over_samples"] = round(mean["combine_records"] / mean["accumulate_records"], 3)
    if "combine_records_never_split" in runs:
        out["split_over_never_split"] = round(mean["combine_records"] / mean["combine_records_never_split"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
