"""Times accumulation inside the renderer's kernel (include/statmc_device_api.hpp) against the arena path it replaces, at the
flagship configuration: 1920 x 1080, 256 samples per pixel, the five stat types of film.STAT_TYPES (11 channels), moments
and arenas from statmc_malloc_placed as bench.py places them.  The renderer is tools/device_accumulate_example.hip's
counter-based hash generator:

  arena  gen_arena writes one film-major arena per type, statmc_accumulate reads them back (what bench.py times)
  fused  gen_fold folds the same values into the moments in registers (statmc::device::PixelStats): no arena

Prints one JSON line per path: milliseconds per step (hipEvent timing, after warm-up; the arena path also split into its two
launches), the algorithmic bytes computed from the shapes, and the share of the 8 TB/s HBM peak they imply.

    python tools/time_device_accumulate.py [--width 1920 --height 1080 --spp 256 --iters 10 --warmup 3] [--slots P | --lanes G,G]

--slots P instead times a renderer with P samples of a pixel in flight, on the radiance type alone (one arena, every pixel's
samples dealt evenly to P slots), and prints two lines:
  merged  fold_arena_slots: every slot folds its share in the kernel, the slots are merged there (PixelStats::merge), one store
  states  P sets of state images, one statmc_accumulate per slot over its share, then one statmc_combine_many

--lanes G[,G...] instead times the generator with several lanes per pixel (statmc::device::merge_lanes) against gen_fold's one
thread per pixel, all five types, no arena, and prints one line per path:
  gen_fold        five timings in this process: their mean is the yardstick, max - min its spread
  gen_fold_lanes  per G: ms and the ratio to the yardstick

Algorithmic bytes: the arena written once and read once (4 B per channel and sample), and the moments read and written once
per step (n, mean, m2, m3, film-mean, film-m2 of radiance; n and mean of the four feature types: 112 B per pixel each way)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, build, film  # noqa: E402

PEAK = 8.0e12
TYPES = ("radiance", "normal", "albedo", "depth", "materialid")   # gen_arena / gen_fold order


def state_bytes_per_pixel():
    b = 0
    for t in TYPES:
        cfg = film.STAT_TYPES[t]
        planes = cfg["max_moment"] + (2 if cfg["transform"] else 0)
        b += 4 + 4 * cfg["channels"] * planes
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


def time_slots(a, dev):
    """--slots: PixelStats::merge inside the kernel against P states + statmc_combine_many (radiance: 3 channels, max_moment 3)."""
    W, H, S, P = a.width, a.height, a.spp, a.slots
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.fold_arena_slots.argtypes = [C.POINTER(api.StatType), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(api.PrepassContext), C.c_void_p]
    cfg = film.STAT_TYPES["radiance"]
    arena = torch.rand(S, H, W, 3, device=dev)
    cuts = [k * S // P for k in range(P + 1)]
    bounds = torch.tensor(cuts, dtype=torch.int32, device=dev)[:, None, None].expand(P + 1, H, W).contiguous()
    states = [film.new_state(H, W, 3, dev, transform=True) for _ in range(P)]
    t = api.make_stat_type(arena, states[0], cfg["transform"], cfg["max_moment"])
    stream = api.current_stream_handle()
    shares = [api.make_stat_type(arena[cuts[k]:cuts[k + 1]], states[k], cfg["transform"], cfg["max_moment"]) for k in range(P)]
    many = [api.make_combine_many_entry(states[0], states[1:], 3, 3)]

    def merged():
        api.check(lib.fold_arena_slots(C.byref(t), W, H, arena.data_ptr(), bounds.data_ptr(), P, None, stream))

    def by_states():
        for k in range(1, P):
            for v in states[k].values():
                v.zero_()
        for st in shares:
            api.accumulate(W, H, [st], stream=stream)
        api.combine_many(W, H, many, stream=stream)

    common = {"width": W, "height": H, "spp": S, "slots": P}
    m_ms = timed(merged, a.iters, a.warmup)
    for st in states:
        for v in st.values():
            v.zero_()
    s_ms = timed(by_states, a.iters, a.warmup)
    print(json.dumps(dict(path="merged", ms=round(m_ms, 4), **common)))
    print(json.dumps(dict(path="states", ms=round(s_ms, 4), merged_speedup=round(s_ms / m_ms, 2), **common)))


def time_lanes(a, dev):
    """--lanes: gen_fold_lanes at each G against gen_fold, placed moments, the five types"""
    W, H, S = a.width, a.height, a.spp
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    gen = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(api.StatType), C.POINTER(api.PrepassContext), C.c_void_p]
    lib.gen_fold.argtypes = gen
    lib.gen_fold_lanes.argtypes = gen[:5] + [C.c_int] + gen[5:]
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    dummy = {t: torch.empty(1, H, W, film.STAT_TYPES[t]["channels"], device=dev) for t in TYPES}   # make_stat_type wants a tensor
    sts = (api.StatType * 5)(*[api.make_stat_type(dummy[t], fs.state[t], film.STAT_TYPES[t]["transform"], film.STAT_TYPES[t]["max_moment"])
                               for t in TYPES])
    stream = api.current_stream_handle()
    step = [0]

    def run(fn, *g):
        def one():
            api.check(fn(1, W, H, step[0] * S, S, *g, sts, None, stream))
            step[0] += 1
        fs.reset()          # counts stay far below 2^24
        step[0] = 0
        return timed(one, a.iters, a.warmup)

    common = {"width": W, "height": H, "spp": S, "iters": a.iters, "warmup": a.warmup, "placed": api.placement_info()["active"] == 1}
    base = [run(lib.gen_fold) for _ in range(5)]
    yard, spread = sum(base) / len(base), max(base) - min(base)
    print(json.dumps(dict(path="gen_fold", ms=round(yard, 4), spread_ms=round(spread, 4), runs_ms=[round(v, 4) for v in base], **common)),
          flush=True)
    for G in a.lanes:
        ms = run(lib.gen_fold_lanes, G)
        print(json.dumps(dict(path="gen_fold_lanes", lanes=G, ms=round(ms, 4), ratio_to_gen_fold=round(ms / yard, 3),
                              beats_yardstick_by_more_than_its_spread=bool(yard - ms > spread), **common)), flush=True)
    again = run(lib.gen_fold)    # the yardstick once more at the end: drift over the process
    print(json.dumps(dict(path="gen_fold_again", ms=round(again, 4), **common)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slots", type=int, default=0, help="P slots per pixel: in-kernel merge against P states + combine_many")
    ap.add_argument("--lanes", type=lambda v: [int(g) for g in v.split(",")], default=None,
                    help="G[,G...] lanes per pixel (2 .. 64, powers of two): gen_fold_lanes against gen_fold")
    a = ap.parse_args()
    W, H, S = a.width, a.height, a.spp
    dev = torch.device("cuda:0")
    api.setup(0)
    build.build_tools()
    if a.slots:
        if not 2 <= a.slots <= api.MAX_COMBINE_SOURCES + 1:
            ap.error("--slots wants 2 .. %d" % (api.MAX_COMBINE_SOURCES + 1))
        return time_slots(a, dev)
    if a.lanes:
        if any(g not in (2, 4, 8, 16, 32, 64) for g in a.lanes):
            ap.error("--lanes wants 2, 4, 8, 16, 32 or 64")
        return time_lanes(a, dev)
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.gen_arena.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    lib.gen_fold.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(api.StatType), C.POINTER(api.PrepassContext),
                             C.c_void_p]
    ch = {t: film.STAT_TYPES[t]["channels"] for t in TYPES}
    api.placement_expect(api.MEM_STREAM, sum(4 * S * H * W * ch[t] for t in TYPES), dev)
    arenas = {t: api.empty_placed((S, H, W, ch[t]), torch.float32, dev, api.MEM_STREAM) for t in TYPES}
    api.placement_expect(api.MEM_STREAM, 0, dev)
    ptrs = (C.c_void_p * 5)(*[arenas[t].data_ptr() for t in TYPES])
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    sts = (api.StatType * 5)(*[api.make_stat_type(arenas[t], fs.state[t], film.STAT_TYPES[t]["transform"], film.STAT_TYPES[t]["max_moment"])
                               for t in TYPES])
    stream = api.current_stream_handle()
    step = [0]

    def gen():
        api.check(lib.gen_arena(1, W, H, step[0] * S, S, ptrs, stream))

    def acc():
        api.accumulate(W, H, list(sts), stream=stream)

    def arena_step():
        gen()
        acc()
        step[0] += 1

    def fused_step():
        api.check(lib.gen_fold(1, W, H, step[0] * S, S, sts, None, stream))
        step[0] += 1

    arena_b = 4 * S * H * W * sum(ch.values())
    state_b = 2 * state_bytes_per_pixel() * H * W
    common = {"width": W, "height": H, "spp": S, "channels": sum(ch.values()), "placed": api.placement_info()["active"] == 1}
    gen_ms, acc_ms = timed(gen, a.iters, a.warmup), timed(acc, a.iters, a.warmup)
    fs.reset()
    arena_ms = timed(arena_step, a.iters, a.warmup)
    b = 2 * arena_b + state_b
    print(json.dumps(dict(path="arena", ms=round(arena_ms, 4), gen_arena_ms=round(gen_ms, 4), accumulate_ms=round(acc_ms, 4),
                          bytes=b, of_peak=round(b / (arena_ms * 1e-3) / PEAK, 3),
                          accumulate_of_peak=round((arena_b + state_b) / (acc_ms * 1e-3) / PEAK, 3), **common)))
    fs.reset()
    fused_ms = timed(fused_step, a.iters, a.warmup)
    print(json.dumps(dict(path="fused", ms=round(fused_ms, 4), bytes=state_b, of_peak=round(state_b / (fused_ms * 1e-3) / PEAK, 3),
                          speedup=round(arena_ms / fused_ms, 2), **common)))


if __name__ == "__main__":
    main()
