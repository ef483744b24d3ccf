"""Times statmc_combine_statistics at 3840 x 2160 (at 1080p part of the working set sits in the 256 MiB Infinity Cache) and
prints one JSON line per state: milliseconds per call (hipEvent timing, after warm-up), the algorithmic bytes computed from
the shapes, and the share of the 8 TB/s HBM peak they imply.

    python tools/time_combine.py [--width 3840 --height 2160 --iters 50 --warmup 10]

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


def entries_of(kind, h, w, dev, gen):
    """[(dst, src, channels, max_moment, count_of)] and the algorithmic bytes of one call."""
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
        out.append((a, b, ch, mm, count_of))
        plane = h * w * ch * 4
        read += 2 * plane * len(fields) + (2 * h * w * 4 if own else 0)
        write += plane * len(fields) + (h * w * 4 if own else 0)
    return out, read, write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--states", default="dump,full")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    W, H = a.width, a.height
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
