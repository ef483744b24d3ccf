"""Times statmc_compact_accumulate -- the compact (CSR) arena: every pixel's samples back to back, pixels in raster order -- against
what a renderer could call instead, at 1920 x 1080 with the five stat types of film.STAT_TYPES (11 channels), sample arenas and
moments from statmc_malloc_placed.  One process per set:

    python tools/time_accumulate_compact.py --set a|b|c|d [--out profiles/accumulate_compact.jsonl --iters 50 --warmup 10 --rounds 5]

  a  16 samples on every pixel.  Yardsticks: statmc_accumulate on the dense (transposed) arena; the records entry in film order.
  b  every pixel its own count, independent and uniform in 1 .. 64.  Yardsticks: statmc_accumulate_counted on the dense arena of
     capacity 64; the records entry.
  c  one sample per pixel plus 16 pixels at 65 536.  Yardstick: statmc_accumulate_records_split with split_above = 256; the compact
     call with split_above = 256 and, as `compact_never_split`, with INT32_MAX.
  d  5 % of the pixels at 256 samples, the others at none.  Yardstick: the records entry.

The records entries get (owners, samples) of statmc_compact_offsets: the same arena, plus 4 bytes of pixel index per sample.  Before
anything is timed the compact call (default dispatch, staged and direct) and the records entry each run once from zeroed moments
and the bits of every state image are compared (`bits_equal`).  Then `rounds` rounds time every entry alternately in this one
process, `iters` calls after `warmup` each (hipEvent timing, moments zeroed before each series); mean over the rounds, spread =
max - min.  "Ahead" / "behind" means beyond 3 x the larger spread.

Per set one JSON line (appended to --out as well): the ms of each entry, the staged-against-direct A/B, and the byte model --
(sum of element bytes) * total + 16 B per pixel of offsets + 2 x the state bytes of the touched pixels -- over the compact call's
time as a share of the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402

PEAK = 8.0e12
STAGE_WAVE_BYTES = 12288      # kStageWaveBytes of statmc_compact.hip: the span of a wave's 64 pixels that the staged kernel takes
TYPES = ("radiance", "normal", "albedo", "depth", "materialid")
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
INT32_MAX = 2 ** 31 - 1


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
    gen = torch.Generator(device=dev).manual_seed(7)
    if which == "a":
        return torch.full((H, W), 16, dtype=torch.int32, device=dev)
    if which == "b":
        return torch.randint(1, 65, (H, W), dtype=torch.int32, device=dev, generator=gen)
    if which == "c":
        c = torch.ones(H * W, dtype=torch.int32, device=dev)
        c[torch.randperm(H * W, device=dev, generator=gen)[:16]] = 65536
        return c.view(H, W)
    c = torch.zeros(H * W, dtype=torch.int32, device=dev)
    c[torch.randperm(H * W, device=dev, generator=gen)[:H * W // 20]] = 256
    return c.view(H, W)


def staged_wave_share(offsets, counts, arena, channels, split_above):
    """The share of the waves with samples that the staged kernel stages for this type, by the kernel's own rule restated on the
    offsets: the span of the wave's 64 pixels, from the 16-byte boundary below its first byte, fits STAGE_WAVE_BYTES and no run in
    it is above split_above.  The other waves of that launch take the direct fold inside the staged kernel."""
    npx = counts.numel()
    edges = torch.arange(0, npx + 64, 64, device=offsets.device).clamp_(max=npx)
    first, last = offsets[edges[:-1]], offsets[edges[1:]]
    size = channels * arena.element_size()
    span = (arena.data_ptr() + first * size) % 16 + (last - first) * size
    longest = torch.nn.functional.pad(counts.view(-1), (0, -npx % 64)).view(-1, 64).max(dim=1).values
    live = last > first
    return round(float(((span <= STAGE_WAVE_BYTES) & (longest <= split_above) & live).sum()) / max(int(live.sum()), 1), 4)


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
    stream = api.current_stream_handle()

    counts = count_map(a.set, W, H, dev)
    total = int(counts.sum())
    touched = int((counts > 0).sum())
    offsets, owners = api.compact_offsets(counts, owners_capacity=total)
    torch.cuda.synchronize()
    assert int(offsets[-1]) == total

    gen = torch.Generator(device=dev).manual_seed(11)
    dense_planes = {"a": 16, "b": 64}.get(a.set, 0)       # the yardsticks' dense arenas share the stream role
    api.placement_expect(api.MEM_STREAM, sum(4 * (total + dense_planes * npx) * ch[t] for t in TYPES), dev)
    arenas = {}
    for t in TYPES:
        arenas[t] = api.empty_placed((total, ch[t]), torch.float32, dev, api.MEM_STREAM)
        arenas[t].copy_(torch.rand((total, ch[t]), device=dev, generator=gen).square_().add_(0.01))
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    compact_types = [api.make_stat_type_compact(arenas[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]
    rec_types = [api.make_stat_type_records(arenas[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]
    split = 256 if a.set == "c" else INT32_MAX

    # the dispatch of an entry's series is pinned once, outside the timed region (run_series): what is timed is the call alone
    pinned = {}

    def compact(path, split_above=split):
        def call():
            api.compact_accumulate(W, H, compact_types, offsets, n_samples=total, split_above=split_above, stream=stream)
        pinned[call] = path
        return call

    def run_series(fn, series):
        api.compact_path(pinned.get(fn, api.COMPACT_PATH_AUTO))
        try:
            return series(fn)
        finally:
            api.compact_path(api.COMPACT_PATH_AUTO)

    runs = {"compact": compact(api.COMPACT_PATH_AUTO), "compact_staged": compact(api.COMPACT_PATH_STAGED), "compact_direct": compact(api.COMPACT_PATH_DIRECT),
            "records": lambda: api.accumulate_records(W, H, rec_types, owners, stream=stream, split_above=256 if a.set == "c" else None)}
    if a.set == "c":
        runs["compact_never_split"] = compact(api.COMPACT_PATH_AUTO, INT32_MAX)
    keep = []
    if a.set in ("a", "b"):     # the dense arena [S][H][W][C]: sample s of pixel p is compact position offsets[p] + s
        S = 16 if a.set == "a" else 64
        slot = (torch.arange(total, device=dev) - offsets[owners.long()]) * npx + owners.long()
        dense_types = []
        for t in TYPES:
            d = api.empty_placed((S, H, W, ch[t]), torch.float32, dev, api.MEM_STREAM)
            d.zero_()
            d.view(S * npx, ch[t])[slot] = arenas[t]
            keep.append(d)
            dense_types.append(api.make_stat_type(d, fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]))
        del slot
        if a.set == "a":
            runs["dense"] = lambda: api.accumulate(W, H, dense_types, stream=stream)
        else:
            runs["counted"] = lambda: api.accumulate(W, H, dense_types, stream=stream, sample_counts=counts)
    api.placement_expect(api.MEM_STREAM, 0, dev)

    def images():
        return [fs.state[t][k] for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    # ---- the same bits as the records entry, on every path
    fs.reset()
    runs["records"]()
    want = [img.clone() for img in images()]
    equal, default_path = True, 0
    for k in ("compact", "compact_staged", "compact_direct"):
        fs.reset()
        run_series(runs[k], lambda fn: fn())
        if k == "compact":
            default_path = api.last_compact_path()
        equal = equal and all(torch.equal(g.view(torch.int32), img.view(torch.int32)) for g, img in zip(want, images()))
    del want
    if not equal:
        print(json.dumps({"set": a.set, "bits_equal": False}), flush=True)
        sys.exit(1)

    # ---- timings, alternating
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            fs.reset()
            ms[k].append(run_series(fn, lambda f: timed(f, a.iters, a.warmup)))
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    model_bytes = 4 * sum(ch.values()) * total + 16 * npx + 2 * state_bytes_per_pixel() * touched
    out = {"set": a.set, "width": W, "height": H, "channels": sum(ch.values()), "total_samples": total, "mean_count": round(total / npx, 3),
           "touched_pixels": touched, "split_above": split, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
           "placed": api.placement_info()["active"] == 1, "default_path": default_path, "bits_equal": True, "model_bytes": model_bytes,
           "compact_of_peak": round(model_bytes / (mean["compact"] * 1e-3) / PEAK, 4)}
    out["staged_wave_share"] = {t: staged_wave_share(offsets, counts, arenas[t], ch[t], split) for t in TYPES}
    for k in runs:
        out[k + "_ms"] = round(mean[k], 4)
        out[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
        out[k + "_runs_ms"] = [round(v, 4) for v in ms[k]]
    out["staged_over_direct"] = round(mean["compact_staged"] / mean["compact_direct"], 3)
    out["compact_over_records"] = round(mean["compact"] / mean["records"], 3)
    for k in ("dense", "counted"):
        if k in runs:
            out["compact_over_" + k] = round(mean["compact"] / mean[k], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
