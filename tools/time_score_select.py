"""Times statmc_score_select and statmc_score_count_above at 1920 x 1080 and 3840 x 2160, in one process, against what a user has
without them and against the library's own planning entry:

  select          1 rank and 8 ranks, on a lognormal score image and on a film of one constant score (every lane of every wave in
                  one bin: the shape wave_match in statmc_select.hip is there for)
  count_above     8 thresholds, lognormal image
  plan_samples    statmc_plan_samples on the same lognormal image: the yardstick of DESIGN.md 4.2c, re-timed here
  floor           one read of `score` (4 B/px) per pass at the copy bandwidth measured in the same process (a device-to-device copy
                  of 512 MiB: bytes read plus bytes written over its time)
  host route      download the score image, np.partition at the ranks, nothing uploaded.  Timed with a host clock around work that
                  begins behind a device synchronise; its values must equal the device's bit for bit.

One JSON line per (size, candidate): milliseconds per call (hipEvent timing, 50 calls after 10, five alternating rounds: every round
times every candidate once; mean over the rounds, and the runs), spread = max - min over the rounds.

    python tools/time_score_select.py [--iters 50 --warmup 10 --rounds 5 --host-runs 3] [--out profiles/score_select.jsonl]
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
import select_reference as ref  # noqa: E402
from statmc_amd import api  # noqa: E402

PASSES = 4          # statmc_select.hip: digits of 8 bits
SIZES = ((1920, 1080), (3840, 2160))
TARGET = 8          # the plan: W H TARGET samples, 1 .. 4 TARGET per pixel


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_score_select.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    bw = copy_bandwidth(dev, 20, 3)
    lines = [json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})]
    for W, H in SIZES:
        px = W * H
        logn = torch.exp(1.5 * torch.randn((H, W), device=dev, generator=gen)).contiguous()
        const = torch.full((H, W), 0.75, dtype=torch.float32, device=dev)
        one = [ref.nearest_rank(0.95, px)]
        eight = [ref.nearest_rank(q, px) for q in (0.5, 0.99, 0.05, 0.95, 1.0, 0.25, 0.75, 0.9)]
        thresholds = [0.01, 0.02, 0.05, 0.1, 0.5, 1.0, 2.0, 10.0]
        ws = torch.empty(api.score_select_workspace(), dtype=torch.uint8, device=dev)
        result = torch.zeros(32, dtype=torch.int64, device=dev)
        above = torch.zeros(8, dtype=torch.int64, device=dev)
        counts = torch.empty((H, W), dtype=torch.int32, device=dev)
        plan_ws = torch.empty(api.plan_samples_workspace(W, H), dtype=torch.uint8, device=dev)
        plan_result = torch.zeros(4, dtype=torch.int64, device=dev)
        sel = lambda img, ranks: (lambda: api.score_select(img, ranks, workspace=ws, result=result))
        cands = {
            "select_1_rank_lognormal": sel(logn, one),
            "select_8_ranks_lognormal": sel(logn, eight),
            "select_1_rank_constant": sel(const, one),
            "select_8_ranks_constant": sel(const, eight),
            "count_above_8_lognormal": lambda: api.score_count_above(logn, thresholds, out=above),
            "plan_samples_lognormal": lambda: api.plan_samples(logn, px * TARGET, 1, 4 * TARGET, out=counts, workspace=plan_ws, result=plan_result),
        }
        runs = {name: [] for name in cands}
        for r in range(a.rounds):                    # alternating: every round times every candidate once
            for name, fn in cands.items():
                runs[name].append(timed(fn, a.iters, a.warmup if r == 0 else 3))
        # the host route, and the proof that both routes select the same values
        got = api.read_select_result(sel(logn, eight)())
        host = []
        for _ in range(a.host_runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keys = ref.keys_of(logn.cpu().numpy())
            values = np.partition(keys, sorted(set(eight)))[eight]
            host.append((time.perf_counter() - t0) * 1e3)
        want = ref.select_ref(logn.cpu().numpy(), eight)
        same = [int(v) for v in values] == got["value_bits"] and all(got[k] == want[k] for k in ref.FIELDS)
        api.score_count_above(logn, thresholds, out=above)
        same = same and [int(c) for c in above.cpu().numpy()] == ref.count_above_ref(logn.cpu().numpy(), thresholds)
        const_got = api.read_select_result(sel(const, eight)())
        same = same and const_got["value_bits"] == [0x3F400000] * 8 and const_got["n_equal"] == [px] * 8
        if not same:
            sys.exit("time_score_select.py: the device's answers differ from the numpy restatement's at %d x %d" % (W, H))
        floor_ms = PASSES * 4 * px / bw * 1e3
        host_ms = sum(host) / len(host)
        mean = {name: sum(v) / len(v) for name, v in runs.items()}
        for name in cands:
            ms = mean[name]
            line = {"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                    "spread_ms": round(max(runs[name]) - min(runs[name]), 4)}
            if name.startswith("select"):
                line.update({"launches": PASSES + 1, "floor_ms": round(floor_ms, 4), "ratio_to_floor": round(ms / floor_ms, 2),
                             "ratio_to_plan_samples": round(ms / mean["plan_samples_lognormal"], 3)})
            if name.endswith("constant"):
                line["ratio_to_lognormal"] = round(ms / mean[name.replace("constant", "lognormal")], 3)
            if name == "select_8_ranks_lognormal":
                line.update({"host_route_ms": round(host_ms, 2), "host_route_runs_ms": [round(x, 2) for x in host],
                             "host_route_over_device": round(host_ms / ms, 1), "same_values_as_host_route": same})
            if name == "count_above_8_lognormal":
                line.update({"floor_ms": round(floor_ms / PASSES, 4), "ratio_to_floor": round(ms / (floor_ms / PASSES), 2)})
            lines.append(json.dumps(line))
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
