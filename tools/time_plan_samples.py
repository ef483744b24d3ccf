"""Times statmc_sample_scores and statmc_plan_samples at 1920 x 1080 and 3840 x 2160 against the two yardsticks a user has:

  host route   what planning costs without these entries: download the score image and n, solve with the numpy restatement of
               include/statmc.h (tests/plan_reference.py: bisection over the level's bit patterns), upload the count image.  Timed
               with a host clock around work that ends in a device synchronise; its counts must equal the device's bit for bit.
  floor        (passes + 3) reads of score and n, 8 B/px each, at the copy bandwidth measured in the same process (a device-to-device
               copy of 512 MiB: bytes read plus bytes written over its time): the five search passes, the block sums and the apply
               read both images, and the apply's write plus the scan make up the last one.

One JSON line per (size, kernel): milliseconds per call (hipEvent timing after warm-up; mean over the rounds, and the runs), the
algorithmic bytes from the shapes, TB/s, and for the plan its ratio to the floor and to the host route.

    python tools/time_plan_samples.py [--iters 100 --warmup 10 --rounds 5 --host-runs 2] [--out profiles/plan_samples.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402

PASSES = 5          # statmc_plan.hip: search passes of 64 candidates each
SIZES = ((1920, 1080), (3840, 2160))
TARGET, FIRST = 8, 8     # the plan: W H TARGET samples, 1 .. 4 TARGET per pixel, after FIRST samples per pixel


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


def copy_bandwidth(dev, iters, warmup):
    """bytes per second of a device-to-device copy far larger than the caches: read + written"""
    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src), iters, warmup)
    return 2 * src.numel() / (ms * 1e-3)


def statistics(W, H, dev, gen):
    """what FIRST samples per pixel of a lognormal radiance leave, roughly: n, film_mean, film_m2 [H, W, 3]"""
    n = torch.full((H, W), FIRST, dtype=torch.int32, device=dev)
    mean = torch.rand((H, W, 3), device=dev, generator=gen) + 0.05
    spread = torch.exp(1.5 * torch.randn((H, W, 1), device=dev, generator=gen))
    m2 = (mean * spread) ** 2 * (FIRST - 1) * (0.5 + torch.rand((H, W, 3), device=dev, generator=gen))
    return n, mean.contiguous(), m2.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_plan_samples.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    bw = copy_bandwidth(dev, 20, 3)
    lines = [json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})]
    for W, H in SIZES:
        px = W * H
        n, mean, m2 = statistics(W, H, dev, gen)
        score = torch.empty((H, W), dtype=torch.float32, device=dev)
        counts = torch.empty((H, W), dtype=torch.int32, device=dev)
        ws = torch.empty(api.plan_samples_workspace(W, H), dtype=torch.uint8, device=dev)
        result = torch.zeros(4, dtype=torch.int64, device=dev)
        budget, c_min, c_max = px * TARGET, 1, 4 * TARGET
        cands = {
            "sample_scores": (lambda: api.sample_scores(n, mean, m2, metric="relative", eps=1e-3, out=score), px * (4 + 12 + 12 + 4)),
            "plan_samples": (lambda: api.plan_samples(score, budget, c_min, c_max, n=n, out=counts, workspace=ws, result=result),
                             px * 8 * (PASSES + 2) + px * 4),
        }
        cands["sample_scores"][0]()
        runs = {name: [] for name in cands}
        for r in range(a.rounds):                    # alternating: every round times every candidate once
            for name, (fn, _) in cands.items():
                runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
        res = api.plan_result_dict(result)
        # the host route, and the proof that both routes plan the same counts
        host = []
        for _ in range(a.host_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_counts, h_res = ref.plan_ref(score.cpu().numpy(), n.cpu().numpy(), budget, c_min, c_max)
            up = torch.from_numpy(h_counts).to(dev)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        same = bool(torch.equal(up, counts)) and all(h_res[k] == res[k] for k in h_res)
        if not same:
            sys.exit("time_plan_samples.py: the device's plan differs from the numpy restatement's at %d x %d" % (W, H))
        floor_ms = (PASSES + 3) * 8 * px / bw * 1e3
        host_ms = sum(host) / len(host)
        for name, (_, nbytes) in cands.items():
            ms = sum(runs[name]) / len(runs[name])
            line = {"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                    "spread_ms": round(max(runs[name]) - min(runs[name]), 4), "bytes": nbytes, "tb_per_s": round(nbytes / (ms * 1e-3) / 1e12, 3)}
            if name == "plan_samples":
                line.update({"launches": PASSES + 3, "budget": budget, "c_min": c_min, "c_max": c_max, "status": res["status"],
                             "level_bits": "0x%08x" % res["level_bits"], "total": res["total"],
                             "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(ms / floor_ms, 2),
                             "host_route_ms": round(host_ms, 1), "host_route_runs_ms": [round(x, 1) for x in host],
                             "host_route_over_device": round(host_ms / ms, 1), "same_counts_as_host_route": same})
            lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
