"""Times statmc_combine_statistics at 3840 x 2160 (at 1080p part of the working set sits in the 256 MiB Infinity Cache) and
prints one JSON line per state: milliseconds per call (hipEvent timing, after warm-up), the algorithmic bytes computed from
the shapes, and the share of the 8 TB/s HBM peak they imply.

    python tools/time_combine.py [--width 3840 --height 2160 --iters 50 --warmup 10] [--parts K]

--parts K (2 .. 16): K parts of each state instead of two, and three lines per state, all timed in this process:
  two_part  one statmc_combine_statistics call (parts 0 and 1), timed five times: the yardstick, with the spread of its runs
  fold      the K - 1 two-part calls that fold parts 1 .. K - 1 into part 0: 3 (K - 1) B bytes for a state of B bytes
  many      one statmc_combine_many call over the same parts: (K + 1) B bytes, and its time relative to the fold's

States:
  dump  the for-ours dump set: radiance n / mean / m2 / m3 (own counts), film and two G-buffer means borrowing them
  full  a whole Estimator: radiance with the raw-sample chain, normal / albedo with their own counts, film borrowing
Algorithmic bytes: per entry, both sides of every combined plane are read and the dst side is written; an entry with its
own counts reads two count images and writes one (borrowed counts are the owner's, read once)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api  # noqa: E402

PEAK = 8.0e12


def state(h, w, ch, fields, own, dev, gen):
    st = {k: torch.rand(h, w, ch, device=dev, generator=gen) for k in fields}
    if own:
        st["n"] = torch.randint(1, 64, (h, w), dtype=torch.int32, device=dev, generator=gen)
    return st


def entries_of(kind, h, w, dev, gen, parts=2):
    """[(dst, src, channels, max_moment, count_of)] and the algorithmic bytes of one two-part call; with parts > 2, src is
    the list of parts 1 .. parts - 1."""
    rad_fields = ("mean", "m2", "m3") + (("film_mean", "film_m2") if kind == "full" else ())
    spec = [("radiance", 3, 3, rad_fields, -1)]
    if kind == "dump":
        spec += [("film", 3, 1, ("mean",), 0), ("normal", 3, 1, ("mean",), 0), ("albedo", 3, 1, ("mean",), 0)]
    else:
        spec += [("normal", 3, 1, ("mean",), -1), ("albedo", 3, 1, ("mean",), -1), ("film", 3, 1, ("mean",), 0)]
    out, read, write = [], 0, 0
    for _, ch, mm, fields, count_of in spec:
        own = count_of < 0
        a, b = state(h, w, ch, fields, own, dev, gen), state(h, w, ch, fields, own, dev, gen)
        if parts > 2:
            b = [b] + [state(h, w, ch, fields, own, dev, gen) for _ in range(parts - 2)]
        out.append((a, b, ch, mm, count_of))
        plane = h * w * ch * 4
        read += 2 * plane * len(fields) + (2 * h * w * 4 if own else 0)
        write += plane * len(fields) + (h * w * 4 if own else 0)
    return out, read, write


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


def time_parts(kind, K, W, H, iters, warmup, dev, gen):
    spec, read, write = entries_of(kind, H, W, dev, gen, parts=K)
    side = write                      # bytes of one part: every plane, and the counts of the owning entries
    assert read == 2 * side
    pair = [[api.make_combine_entry(d, ss[k], ch, mm, count_of=c) for d, ss, ch, mm, c in spec] for k in range(K - 1)]
    many = [api.make_combine_many_entry(d, ss, ch, mm, count_of=c) for d, ss, ch, mm, c in spec]

    def fold():
        for es in pair:
            api.combine_statistics(W, H, es)

    common = {"state": kind, "parts": K, "width": W, "height": H, "part_bytes": side}
    line = lambda kernel, ms, b, **kw: print(json.dumps(dict(
        common, kernel=kernel, ms=round(ms, 4), bytes=b, tb_per_s=round(b / (ms * 1e-3) / 1e12, 3),
        of_peak=round(b / (ms * 1e-3) / PEAK, 4), **kw)), flush=True)
    runs = [timed(lambda: api.combine_statistics(W, H, pair[0]), iters, warmup) for _ in range(5)]
    two_ms = sum(runs) / len(runs)
    shares = [3 * side / (ms * 1e-3) / PEAK for ms in runs]
    line("two_part", two_ms, 3 * side, runs_ms=[round(r, 4) for r in runs], spread_ms=round(max(runs) - min(runs), 4),
         spread_of_peak=round(max(shares) - min(shares), 4))
    fold_ms = timed(fold, iters, warmup)
    line("fold", fold_ms, 3 * (K - 1) * side, calls=K - 1)
    many_ms = timed(lambda: api.combine_many(W, H, many), iters, warmup)
    line("many", many_ms, (K + 1) * side, ratio_to_fold=round(many_ms / fold_ms, 4), byte_model_ratio=round((K + 1) / (3 * (K - 1)), 4))
    del spec, pair, many
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--states", default="dump,full")
    ap.add_argument("--parts", type=int, default=0, help="K parts: the fold of K - 1 two-part calls against one statmc_combine_many")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    W, H = a.width, a.height
    if a.parts:
        if not 2 <= a.parts <= api.MAX_COMBINE_SOURCES + 1:
            ap.error("--parts wants 2 .. %d" % (api.MAX_COMBINE_SOURCES + 1))
        for kind in a.states.split(","):
            time_parts(kind, a.parts, W, H, a.iters, a.warmup, dev, gen)
        return
    for kind in a.states.split(","):
        spec, read, write = entries_of(kind, H, W, dev, gen)
        es = [api.make_combine_entry(d, s, ch, mm, count_of=c) for d, s, ch, mm, c in spec]
        for _ in range(a.warmup):
            api.combine_statistics(W, H, es)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            api.combine_statistics(W, H, es)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.iters
        total = read + write
        print(json.dumps({"state": kind, "width": W, "height": H, "ms": round(ms, 4), "read_bytes": read, "write_bytes": write,
                          "bytes_per_pixel": total / (W * H), "tb_per_s": round(total / (ms * 1e-3) / 1e12, 3),
                          "of_peak": round(total / (ms * 1e-3) / PEAK, 3)}))
        del spec, es
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
