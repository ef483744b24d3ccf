"""Times statmc_accumulate_records -- samples handed in as unordered (pixel, sample) records -- against the arena path on the
same samples, at 1920 x 1080 with the five stat types of film.STAT_TYPES (11 channels) and moments from
statmc_malloc_placed.  The values come from tools/device_accumulate_example.hip's hash generator (gen_arena), so the
yardstick sees the same samples.  One process per record set:

    python tools/time_accumulate_records.py --set a|b|c [--width 1920 --height 1080 --iters 50 --warmup 10]

  a  16 records for every pixel; the records of sample s visit the pixels in a shuffled order of their own
  b  the same records in film order: record s * W * H + p belongs to pixel p (the arena itself, read record-major)
  c  sparse: 5 % of the pixels at 256 records each, the pixels of sample s in a shuffled order of their own

Per set, one JSON line: the whole call, its grouping step and its fold alone (statmc_debug_accumulate_records_phases; hipEvent
timing, `iters` calls after `warmup`), the fold's and the call's rate against the byte model and the share of the 8 TB/s HBM
peak, and the yardstick: statmc_accumulate on a film-major arena of S = max count planes, timed five times in this process
(mean = yardstick, max - min = spread).  Before anything is timed the records path and the arena path each run once from
zeroed moments and the bits of every state image are compared on the pixels that have records (`bits_equal_to_arena`).

Byte model of the fold: 4 + 4 * 11 bytes per record, plus 8 B of order[] traffic per record, plus the state of the touched
pixels read and written (2 * 112 B per pixel).  The grouping's own traffic (the sort's passes over 8 B pairs) is not in it."""
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


def placed_copy(t, dev):
    out = api.empty_placed(tuple(t.shape), t.dtype, dev, api.MEM_STREAM)
    out.copy_(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("a", "b", "c"), required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    S = 256 if a.set == "c" else 16
    dev = torch.device("cuda:0")
    api.setup(0)
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.gen_arena.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    ch = {t: film.STAT_TYPES[t]["channels"] for t in TYPES}
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = api.current_stream_handle()

    # ---- the samples: the dense arena of S planes (the yardstick's input), and the record set drawn from it
    api.placement_expect(api.MEM_STREAM, sum(4 * S * npx * ch[t] for t in TYPES), dev)
    arenas = {t: api.empty_placed((S, H, W, ch[t]), torch.float32, dev, api.MEM_STREAM) for t in TYPES}
    api.placement_expect(api.MEM_STREAM, 0, dev)
    ptrs = (C.c_void_p * 5)(*[arenas[t].data_ptr() for t in TYPES])
    api.check(lib.gen_arena(1, W, H, 0, S, ptrs, stream))
    torch.cuda.synchronize()
    if a.set == "b":
        pixels = torch.arange(npx, dtype=torch.int32, device=dev).repeat(S)
        samples = {t: arenas[t].view(S * npx, ch[t]) for t in TYPES}
        touched = torch.ones(npx, dtype=torch.bool, device=dev)
    else:
        if a.set == "a":
            subset = torch.arange(npx, device=dev)
        else:
            subset = torch.randperm(npx, device=dev, generator=gen)[:npx // 20]
        idx = torch.stack([subset[torch.randperm(subset.numel(), device=dev, generator=gen)] for _ in range(S)])   # [S, k]
        plane = torch.arange(S, device=dev)[:, None]
        pixels = idx.to(torch.int32).reshape(-1).contiguous()
        samples = {t: placed_copy(arenas[t].view(S, npx, ch[t])[plane, idx].reshape(-1, ch[t]), dev) for t in TYPES}
        touched = torch.zeros(npx, dtype=torch.bool, device=dev)
        touched[subset] = True
        del idx
    n_rec = pixels.numel()
    n_touched = int(touched.sum())

    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    cfg = film.STAT_TYPES
    rec_types = [api.make_stat_type_records(samples[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]
    arena_types = [api.make_stat_type(arenas[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    def records():
        api.accumulate_records(W, H, rec_types, pixels, stream=stream)

    def arena():
        api.accumulate(W, H, arena_types, stream=stream)

    def phases(p):
        api.check(api.load().statmc_debug_accumulate_records_phases(p))

    def images():
        return [fs.state[t][k] for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    # ---- the same bits as the arena path, on the pixels that have records
    fs.reset()
    records()
    got = [img.reshape(npx, -1)[touched].clone() for img in images()]
    fs.reset()
    arena()
    equal = all(torch.equal(g.view(torch.int32), img.reshape(npx, -1)[touched].view(torch.int32)) for g, img in zip(got, images()))
    del got

    # ---- timings; the moments are zeroed before each series, so counts stay far below 2^24
    fs.reset()
    call_ms = timed(records, a.iters, a.warmup)
    phases(1)
    group_ms = timed(records, a.iters, a.warmup)
    phases(2)
    fs.reset()
    fold_ms = timed(records, a.iters, a.warmup)     # over the index the grouping-only calls left in the workspace
    phases(3)
    yard = []
    for _ in range(5):
        fs.reset()
        yard.append(timed(arena, a.iters, a.warmup))
    yard_ms, spread = sum(yard) / len(yard), max(yard) - min(yard)

    sum_c = sum(ch.values())
    state_b = 2 * state_bytes_per_pixel()
    fold_bytes = n_rec * (4 + 4 * sum_c + 8) + n_touched * state_b
    arena_bytes = 4 * S * npx * sum_c + npx * state_b
    share = lambda b, ms: round(b / (ms * 1e-3) / PEAK, 4)
    print(json.dumps({
        "set": a.set, "width": W, "height": H, "records": n_rec, "records_per_touched_pixel": S, "touched_pixels": n_touched,
        "channels": sum_c, "iters": a.iters, "warmup": a.warmup, "placed": api.placement_info()["active"] == 1,
        "bits_equal_to_arena": bool(equal),
        "call_ms": round(call_ms, 4), "grouping_ms": round(group_ms, 4), "fold_ms": round(fold_ms, 4),
        "fold_bytes": fold_bytes, "fold_tb_per_s": round(fold_bytes / (fold_ms * 1e-3) / 1e12, 3), "fold_of_peak": share(fold_bytes, fold_ms),
        "call_of_peak": share(fold_bytes, call_ms),
        "arena_planes": S, "arena_bytes": arena_bytes, "arena_ms": round(yard_ms, 4), "arena_spread_ms": round(spread, 4),
        "arena_runs_ms": [round(v, 4) for v in yard], "arena_of_peak": share(arena_bytes, yard_ms),
        "call_over_arena": round(call_ms / yard_ms, 3), "fold_over_arena": round(fold_ms / yard_ms, 3),
    }), flush=True)


if __name__ == "__main__":
    main()
