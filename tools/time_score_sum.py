"""Times statmc_score_sum at 1920 x 1080 and 3840 x 2160, in one process, against the library's own one-pass yardstick and against
what a host has without it:

  score_sum       1 cap (+inf) and 4 caps (0.05, +inf, 1, 0.01), on
                    random_exponent   every exponent equally likely: a lane's run (statmc_score_sum.hip) ends at nearly every pixel
                    error_scores      statmc_error_scores of random statistics, 2 to 9 samples per pixel, some below 2 (+inf)
                    constant          one score everywhere: every lane on the same limbs, one run per lane
  count_above     statmc_score_count_above with 1 and 4 thresholds on the random image, in the same rounds: one pass over the same
                  bytes with integer atomics
  floor           one read of `score` (4 B/px) at the copy bandwidth measured in the same process (a device-to-device copy of
                  512 MiB: bytes read plus bytes written over its time)
  host route      download the score image and add it up in float64 with numpy.  Timed with a host clock around work that begins
                  behind a device synchronise.

Nothing is reported unless every timed configuration equals the restatement in Python integers (tests/score_sum_reference.py) bit
for bit.  One JSON line per (size, candidate): milliseconds per call (hipEvent timing, 50 calls after 10, five alternating rounds:
every round times every candidate once; mean over the rounds, and the runs), spread = max - min over the rounds.

    python tools/time_score_sum.py [--iters 50 --warmup 10 --rounds 5 --host-runs 3] [--out profiles/score_sum.jsonl]
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
import score_sum_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402

SIZES = ((1920, 1080), (3840, 2160))
CAPS = {1: [float("inf")], 4: [0.05, float("inf"), 1.0, 0.01]}


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


def images(W, H, dev, gen):
    bits = (torch.randint(1, 255, (H, W), device=dev, generator=gen, dtype=torch.int32) << 23) | torch.randint(0, 1 << 23, (H, W), device=dev,
                                                                                                               generator=gen, dtype=torch.int32)
    n = torch.randint(2, 10, (H, W), device=dev, generator=gen, dtype=torch.int32)
    n.view(-1)[::97] = 1
    mean = torch.rand((H, W, 3), device=dev, generator=gen)
    m2 = torch.rand((H, W, 3), device=dev, generator=gen) * n.unsqueeze(-1) * 0.05
    return {"random_exponent": bits.view(torch.float32).contiguous(),
            "error_scores": api.error_scores(n, mean.contiguous(), m2.contiguous(), metric="relative", eps=1e-3, table="stderr"),
            "constant": torch.full((H, W), 0.75, dtype=torch.float32, device=dev)}


def whole(r):
    return ref.result_bits({**r, **{f: list(r[f]) + [0] * (4 - len(r[f])) for f in ("cap_bits", "n_clipped", "sum", "sum_sq")}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score_sum.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    bw = copy_bandwidth(dev, 20, 3)
    lines = [json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})]
    for W, H in SIZES:
        px = W * H
        imgs = images(W, H, dev, gen)
        ws = torch.empty(api.score_sum_workspace(), dtype=torch.uint8, device=dev)
        result = torch.zeros(19, dtype=torch.int64, device=dev)
        above = torch.zeros(4, dtype=torch.int64, device=dev)
        cands = {}
        for k, caps in CAPS.items():
            for name, img in imgs.items():
                cands["score_sum_%d_%s" % (k, name)] = (lambda img=img, caps=caps: api.score_sum(img, caps, workspace=ws, result=result))
            cands["count_above_%d_random_exponent" % k] = (lambda caps=caps, k=k: api.score_count_above(imgs["random_exponent"], caps, out=above[:k]))
        # every timed configuration against the restatement, before anything is timed
        for k, caps in CAPS.items():
            for name, img in imgs.items():
                got = api.read_sum_result(cands["score_sum_%d_%s" % (k, name)]())
                want = ref.sum_ref(img.cpu().numpy(), caps)
                if whole(got) != ref.result_bits(want):
                    sys.exit("time_score_sum.py: %s with %d caps differs from the restatement at %d x %d" % (name, k, W, H))
        runs = {name: [] for name in cands}
        for r in range(a.rounds):                    # alternating: every round times every candidate once
            for name, fn in cands.items():
                runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
        host = []
        for _ in range(a.host_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            total = float(np.sum(imgs["constant"].cpu().numpy(), dtype=np.float64))
            host.append((time.perf_counter() - t0) * 1e3)
        assert total == 0.75 * px
        floor_ms = 4 * px / bw * 1e3
        host_ms = sum(host) / len(host)
        mean = {name: sum(v) / len(v) for name, v in runs.items()}
        spread = {name: max(v) - min(v) for name, v in runs.items()}
        for name in cands:
            ms = mean[name]
            line = {"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                    "spread_ms": round(spread[name], 4), "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(ms / floor_ms, 2)}
            if name.startswith("score_sum"):
                k = name.split("_")[2]
                yard = "count_above_%s_random_exponent" % k
                line.update({"launches": 2, "ratio_to_count_above": round(ms / mean[yard], 3),
                             "behind_count_above_in_spreads": round((ms - mean[yard]) / max(spread[name], spread[yard], 1e-4), 1),
                             "equals_the_restatement": True})
                if not name.endswith("random_exponent"):
                    rnd = "score_sum_%s_random_exponent" % k
                    line["behind_random_exponent_in_spreads"] = round((ms - mean[rnd]) / max(spread[name], spread[rnd], 1e-4), 1)
            if name == "score_sum_1_constant":
                line.update({"host_route_ms": round(host_ms, 2), "host_route_runs_ms": [round(x, 2) for x in host],
                             "host_route_over_device": round(host_ms / ms, 1)})
            lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
