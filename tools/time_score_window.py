"""Times statmc_score_window at 1920 x 1080 and 3840 x 2160, in one process, against the library's own pointwise pass and against
what a user has without it:

  window          MAX and MIN at radius 1, 5, 20 and 32, on a lognormal score image and on a film of one constant score
  sample_scores   statmc_sample_scores (3 channels, relative metric): a pointwise pass of comparable bytes -- the price of a launch
                  that only streams the film; every window line carries its ratio to it
  max_pool2d      torch.nn.functional.max_pool2d with the same window (stride 1, padding r) on the same lognormal image; its
                  values must equal the device's bit for bit
  floor           one read and one write of the film (8 B/px) at the copy bandwidth measured in the same process (a
                  device-to-device copy of 512 MiB: bytes read plus bytes written over its time)
  host route      download the score image, the separable numpy restatement, upload the result.  Timed with a host clock around
                  work that begins behind a device synchronise; its values must equal the device's bit for bit.

Everything runs on one library stream (statmc_stream_create), events recorded on it.  One JSON line per (size, candidate):
milliseconds per call (50 calls after 10, five alternating rounds: every round times every candidate once; mean over the rounds,
and the runs), spread = max - min over the rounds.

    python tools/time_score_window.py [--iters 50 --warmup 10 --rounds 5 --host-runs 2] [--out profiles/score_window.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import score_window_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402

SIZES = ((1920, 1080), (3840, 2160))
RADII = (1, 5, 20, 32)
HOST_RADIUS = 5     # the host route's window


def timed(fn, iters, warmup, stream):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(iters):
        fn()
    t1.record(stream)
    stream.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score_window.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    lib = api.load()
    handle = C.c_void_p()
    api.check(lib.statmc_stream_create(C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value, device=dev)
    lines = []
    try:
        with torch.cuda.stream(stream):      # api.* and torch both enqueue on the library stream
            gen = torch.Generator(device=dev).manual_seed(1)
            src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)
            dst = torch.empty_like(src)
            bw = 2 * src.numel() / (timed(lambda: dst.copy_(src), 20, 3, stream) * 1e-3)
            del src, dst
            lines.append(json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)}))
            for W, H in SIZES:
                px = W * H
                logn = torch.exp(1.5 * torch.randn((H, W), device=dev, generator=gen)).contiguous()
                const = torch.full((H, W), 0.75, dtype=torch.float32, device=dev)
                out = torch.empty((H, W), dtype=torch.float32, device=dev)
                n = torch.full((H, W), 8, dtype=torch.int32, device=dev)
                mean = torch.rand((H, W, 3), device=dev, generator=gen)
                m2 = torch.rand((H, W, 3), device=dev, generator=gen)
                cands = {"sample_scores": lambda: api.sample_scores(n, mean, m2, out=out)}
                for r in RADII:
                    for op in ("max", "min"):
                        for name, img in (("lognormal", logn), ("constant", const)):
                            cands["window_%s_r%d_%s" % (op, r, name)] = (lambda img=img, r=r, op=op: api.score_window(img, r, op, out=out))
                    cands["max_pool2d_r%d_lognormal" % r] = (lambda r=r: torch.nn.functional.max_pool2d(logn[None, None], 2 * r + 1, 1, r))
                runs = {name: [] for name in cands}
                for rnd in range(a.rounds):                  # alternating: every round times every candidate once
                    for name, fn in cands.items():
                        runs[name].append(timed(fn, a.iters, a.warmup if rnd == 0 else 3, stream))
                # the same bits by all three routes
                same = True
                for r in RADII:
                    got = api.score_window(logn, r, "max")
                    same = same and torch.equal(got.view(torch.int32), torch.nn.functional.max_pool2d(logn[None, None], 2 * r + 1, 1, r)[0, 0].view(torch.int32))
                host = []
                for _ in range(a.host_runs):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    up = torch.from_numpy(ref.window_ref(logn.cpu().numpy(), ref.MAX, HOST_RADIUS)).to(dev)
                    stream.synchronize()
                    host.append((time.perf_counter() - t0) * 1e3)
                same = same and torch.equal(up.view(torch.int32), api.score_window(logn, HOST_RADIUS, "max").view(torch.int32))
                same = same and bool((api.score_window(const, 32, "min") == 0.75).all())
                if not same:
                    sys.exit("time_score_window.py: the device's windows differ from max_pool2d's or the numpy restatement's at %d x %d" % (W, H))
                floor_ms = 8 * px / bw * 1e3
                host_ms = sum(host) / len(host)
                avg = {name: sum(v) / len(v) for name, v in runs.items()}
                for name in cands:
                    ms = avg[name]
                    line = {"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                            "spread_ms": round(max(runs[name]) - min(runs[name]), 4)}
                    if name.startswith("window"):
                        r = int(name.split("_")[2][1:])
                        line.update({"radius": r, "ratio_to_sample_scores": round(ms / avg["sample_scores"], 2), "floor_ms": round(floor_ms, 4),
                                     "ratio_to_r1": round(ms / avg[name.replace("_r%d_" % r, "_r1_")], 2)})
                        if name.startswith("window_max") and name.endswith("lognormal"):
                            line["ratio_to_max_pool2d"] = round(ms / avg["max_pool2d_r%d_lognormal" % r], 3)
                        if name == "window_max_r%d_lognormal" % HOST_RADIUS:
                            line.update({"host_route_ms": round(host_ms, 2), "host_route_runs_ms": [round(x, 2) for x in host],
                                         "host_route_over_device": round(host_ms / ms, 1), "same_bits_as_max_pool2d_and_host_route": same})
                    lines.append(json.dumps(line))
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_stream_destroy(handle))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
