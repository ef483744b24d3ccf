"""Times statmc_accumulate_counted -- the dense arena plus an int32 image of per-pixel sample counts -- against what a renderer
could call instead, at 1920 x 1080 with the five stat types of film.STAT_TYPES (11 channels), an arena of capacity S = 64 and
moments from statmc_malloc_placed.  The values come from tools/device_accumulate_example.hip's hash generator (gen_arena).  One
process per count map:

    python tools/time_accumulate_counted.py --map u|t|p [--out profiles/accumulate_counted.jsonl --iters 20 --warmup 5 --rounds 5]

  u  every count 64.  Yardstick: statmc_accumulate on the same arena.
  t  one count per 16 x 16 tile: 64 on every fourth tile, 4 on the rest.
  p  every pixel its own count, independent and uniform in 1 .. 64.

For t and p there are two yardsticks: statmc_accumulate_records on exactly the live samples (its input -- the records in
sample-major order, ascending s inside a pixel -- is built outside the timed region), and statmc_accumulate over all 64 planes,
the cost of ignoring the counts.  Before anything is timed the counted call and the yardstick that defines it (u: statmc_accumulate,
t / p: statmc_accumulate_records) each run once from zeroed moments and the bits of every state image are compared
(`bits_equal`).  Then `rounds` rounds time the counted call and its yardsticks alternately, `iters` calls after `warmup` each
(hipEvent timing, moments zeroed before each series); mean over the rounds, spread = max - min.

Per map one JSON line (appended to --out as well): the ms of each, the ratios, and the live bytes -- 44 B per live pixel-sample
plus the state of the touched pixels read and written, 2 * 112 B each -- over the counted call's time as a share of the 8 TB/s
HBM peak."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, build, film  # noqa: E402

PEAK = 8.0e12
TYPES = ("radiance", "normal", "albedo", "depth", "materialid")   # gen_arena order
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
S = 64


def state_bytes_per_pixel():
    b = 0
    for t in TYPES:
        cfg = film.STAT_TYPES[t]
        b += 4 + 4 * cfg["channels"] * (cfg["max_moment"] + (2 if cfg["transform"] else 0))
    return b


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


def count_map(which, W, H, dev):
    if which == "u":
        return torch.full((H, W), S, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    if which == "t":
        ty, tx = (H + 15) // 16, (W + 15) // 16
        tile = torch.where(torch.arange(ty * tx, device=dev) % 4 == 0, S, 4).to(torch.int32).view(ty, tx)
        return tile.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W].contiguous()
    return torch.randint(1, S + 1, (H, W), dtype=torch.int32, device=dev, generator=gen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", choices=("u", "t", "p"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON line to this file as well")
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    dev = torch.device("cuda:0")
    api.setup(0)
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.gen_arena.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    ch = {t: film.STAT_TYPES[t]["channels"] for t in TYPES}
    stream = api.current_stream_handle()

    api.placement_expect(api.MEM_STREAM, sum(4 * S * npx * ch[t] for t in TYPES), dev)
    arenas = {t: api.empty_placed((S, H, W, ch[t]), torch.float32, dev, api.MEM_STREAM) for t in TYPES}
    api.placement_expect(api.MEM_STREAM, 0, dev)
    ptrs = (C.c_void_p * 5)(*[arenas[t].data_ptr() for t in TYPES])
    api.check(lib.gen_arena(1, W, H, 0, S, ptrs, stream))
    torch.cuda.synchronize()

    counts = count_map(a.map, W, H, dev)
    sum_c = int(counts.sum())
    touched = int((counts > 0).sum())
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    cfg = film.STAT_TYPES
    arena_types = [api.make_stat_type(arenas[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    def counted():
        api.accumulate(W, H, arena_types, stream=stream, sample_counts=counts)

    def full():
        api.accumulate(W, H, arena_types, stream=stream)

    runs = {"counted": counted, "all_planes": full}
    if a.map != "u":    # the live samples as records, sample-major: ascending s inside every pixel
        live = torch.arange(S, device=dev, dtype=torch.int32)[:, None] < counts.view(1, npx)      # [S, npx]
        pixels = live.nonzero()[:, 1].to(torch.int32).contiguous()
        samples = {}
        for t in TYPES:
            rec = arenas[t].view(S, npx, ch[t])[live]
            samples[t] = api.empty_placed(tuple(rec.shape), torch.float32, dev, api.MEM_STREAM)
            samples[t].copy_(rec)
            del rec
        del live
        assert pixels.numel() == sum_c
        rec_types = [api.make_stat_type_records(samples[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]
        runs["records"] = lambda: api.accumulate_records(W, H, rec_types, pixels, stream=stream)

    def images():
        return [fs.state[t][k] for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    # ---- the same bits as the yardstick that defines the call
    fs.reset()
    counted()
    path = api.last_accumulate_counted()
    got = [img.clone() for img in images()]
    fs.reset()
    runs["all_planes" if a.map == "u" else "records"]()
    equal = all(torch.equal(g.view(torch.int32), img.view(torch.int32)) for g, img in zip(got, images()))
    del got
    if not equal:
        print(json.dumps({"map": a.map, "bits_equal": False}), flush=True)
        sys.exit(1)

    # ---- timings, alternating
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            fs.reset()
            ms[k].append(timed(fn, a.iters, a.warmup))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    live_bytes = 4 * sum(ch.values()) * sum_c + 2 * state_bytes_per_pixel() * touched
    out = {"map": a.map, "width": W, "height": H, "capacity": S, "channels": sum(ch.values()), "sum_counts": sum_c, "mean_count": round(sum_c / npx, 3),
           "touched_pixels": touched, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds, "placed": api.placement_info()["active"] == 1,
           "path": {1: "vector", 2: "element"}.get(path, "none"), "bits_equal": True, "live_bytes": live_bytes,
           "counted_of_peak": round(live_bytes / (mean["counted"] * 1e-3) / PEAK, 4)}
    for k in runs:
        out[k + "_ms"] = round(mean[k], 4)
        out[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
        out[k + "_runs_ms"] = [round(v, 4) for v in ms[k]]
    out["counted_over_all_planes"] = round(mean["counted"] / mean["all_planes"], 3)
    if "records" in runs:
        out["counted_over_records"] = round(mean["counted"] / mean["records"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
