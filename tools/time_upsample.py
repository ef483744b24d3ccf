"""Times statmc_upsample_filtered and the preview path built on it, in one process:

  launch   the upsample launch alone at 1920 x 1080 and 3840 x 2160, k = 2, 4, 8, RGB with two RGB G-buffers, on a denoised pooled
           synthetic film.  floor: its algorithmic bytes -- 72 B per fine pixel in and out plus the 72 B coarse set of one pixel per
           k x k block -- at the copy bandwidth measured in the same process.  statmc_prepass on the fine film is timed in the same
           rounds: a pointwise launch of similar traffic (64 B/px), and the yardstick for the launch's distance from its floor.
  preview  FilmStats.preview(k) -- pool, coarse pre-pass (the pool's epilogue) and window filter, upsample; the fine pre-pass is the
           accumulation's epilogue -- against statmc_filter_f32x3 on the fine film, at r = 20 and r = 6.
  quality  recorded, not judged: at 960 x 540 and 4, 16 and 64 spp the relative L2 against the scene's expectation of the noisy
           film, the full filter's result and the preview at k = 2 and k = 4.

Refuses to report unless, for every timed launch configuration, the device's image equals the numpy restatement's
(tests/upsample_reference.py) bit for bit with the factors at 0, and with the timed factors stays within 1e-5 relative L2 per channel of
the float64 evaluation with the restatement's fallback mask (pixels whose member weights all lie under the float32 normal range are
counted and left out of that second check: the float32 definition keeps only a few bits of their quotient).  Everything runs on one library stream (statmc_stream_create), events
recorded on it.  One JSON line per candidate: milliseconds per call (50 calls after 10, five alternating rounds: every round times
every candidate once; mean over the rounds, and the runs), spread = max - min over the rounds.

    python tools/time_upsample.py [--iters 50 --warmup 10 --rounds 5] [--out profiles/upsample.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import upsample_reference as ref  # noqa: E402
from statmc_amd import api, film, synthetic  # noqa: E402

SIZES = ((1920, 1080), (3840, 2160))
KS = (2, 4, 8)
SPP = 8
FIREFLY = 1.0 + 999.0 * 5e-4      # synthetic.Scene.samples: a sample is 1000 x with probability 5e-4; the rest of its factors have mean 1


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


def make_film(W, H, spp, dev, radius=20, batch=8):
    scene = synthetic.Scene(W, H, n_regions=12, seed=1, device=dev)
    fs = film.FilmStats(W, H, dev, radius=radius, fused_prepass=True)
    done = 0
    while done < spp:
        s = min(batch, spp - done)
        fs.accumulate(scene.samples(s, seed=100 + done, features=("radiance", "normal", "albedo")))
        done += s
    return scene, fs


def host(t):
    return t.cpu().numpy()


def check_launch(fs, coarse, k, g_dr, who):
    """the two checks of tests/test_upsample_gpu.py on the film that is timed"""
    fine_h = dict(mean_corr=host(fs.mean_corr), disc=host(fs.disc), colour=host(fs.state["radiance"]["film_mean"]),
                  g=[host(fs.g_buffer(g)) for g in fs.g_names])
    coarse_h = dict(mean_corr=host(coarse.mean_corr), disc=host(coarse.disc), filtered=host(coarse.film_f),
                    g=[host(coarse.g_buffer(g)) for g in coarse.g_names])
    spec = api.get_filter_spec()
    for factors in ([0.0] * len(g_dr), list(g_dr)):
        fa, keep_f = fs.filter_args()
        ca, keep_c = coarse.filter_args()
        dr = (C.c_float * len(factors))(*factors)
        fa.g_dr_factors = ca.g_dr_factors = dr
        api.upsample_filtered(fa, ca, k, 3)
        got = host(fs.film_f)
        want = ref.upsample_ref(fine_h, coarse_h, k, spec.gate, spec.channel_rule, spec.border, factors, fma=ref.fmaf_fast)
        own = (got.view(np.uint32) == fine_h["colour"].view(np.uint32)).all(-1)
        if any(factors):
            # a pixel all of whose member weights lie under the float32 normal range (every candidate far away in feature space: e
            # below -87) has a float32 sum of a few bits, or none where the exponential flushes: the definition itself loses the
            # quotient there.  Such pixels are counted and left out of the float64 comparison; everywhere else both checks hold.
            with np.errstate(all="ignore"):
                tiny = ~want["fallback"] & (want["sum64"] < 2.0 ** -100)
            keep = ~tiny
            err = max(float(np.sqrt(((got[..., c] - want["out64"][..., c])[keep] ** 2).sum() / (want["out64"][..., c][keep] ** 2).sum())) for c in range(3))
            if not err <= 1e-5 or not np.array_equal(own[keep], want["fallback"][keep]):
                sys.exit("time_upsample.py: %s: %.3g relative L2 against the float64 evaluation, or another fallback mask" % (who, err))
        elif not np.array_equal(got.view(np.uint32), want["out"].view(np.uint32)):
            sys.exit("time_upsample.py: %s: with the factors at 0 the device's bits differ from the restatement's" % who)
    return float(want["fallback"].mean()), float(want["member"].mean()), err, int(tiny.sum())


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: launch, preview, quality")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    if not torch.cuda.is_available():
        sys.exit("time_upsample.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    lib = api.load()
    handle = C.c_void_p()
    api.check(lib.statmc_stream_create(C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value, device=dev)
    lines = []

    def rounds(cands):
        runs = {name: [] for name in cands}
        for rnd in range(a.rounds):                  # alternating: every round times every candidate once
            for name, fn in cands.items():
                runs[name].append(timed(fn, a.iters, a.warmup if rnd == 0 else 3, stream))
        return runs

    def entry(name, W, H, runs, **more):
        v = runs[name]
        line = {"kernel": name, "width": W, "height": H, "ms": round(sum(v) / len(v), 4), "runs_ms": [round(x, 4) for x in v],
                "spread_ms": round(max(v) - min(v), 4)}
        line.update(more)
        return line

    try:
        with torch.cuda.stream(stream):      # api.* and torch both enqueue on the library stream
            src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)
            dst = torch.empty_like(src)
            bw = 2 * src.numel() / (timed(lambda: dst.copy_(src), 20, 3, stream) * 1e-3)
            del src, dst
            lines.append({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)})
            for W, H in SIZES:
                if {"launch", "preview"} <= skip:
                    break
                px = W * H
                scene, fs = make_film(W, H, SPP, dev)
                g_dr = [-0.5 / (sd * sd) for sd in fs.g_sds]
                # ---- the launch alone
                if "launch" not in skip:
                    cands, keep, facts = {}, [], {}
                    pa, keep_p = fs.filter_args()
                    cands["prepass"] = lambda: api.prepass(pa, 3)
                    for k in KS:
                        coarse = fs.pooled(k)
                        coarse.denoise()
                        fs.prepass()
                        facts[k] = check_launch(fs, coarse, k, g_dr, "%d x %d, k = %d" % (W, H, k))
                        fa, keep_f = fs.filter_args()
                        ca, keep_c = coarse.filter_args()
                        keep.append((coarse, fa, ca, keep_f, keep_c))
                        cands["upsample_k%d" % k] = (lambda fa=fa, ca=ca, k=k: api.upsample_filtered(fa, ca, k, 3))
                    runs = rounds(cands)
                    pre = entry("prepass", W, H, runs, bytes_per_px=64, floor_ms=round(64 * px / bw * 1e3, 4))
                    pre["over_floor"] = round(pre["ms"] / pre["floor_ms"], 3)
                    lines.append(pre)
                    for k in KS:
                        b = 72 + 72.0 / (k * k)
                        e = entry("upsample_k%d" % k, W, H, runs, bytes_per_px=round(b, 3), floor_ms=round(b * px / bw * 1e3, 4), checked=True,
                                  fallback_share=round(facts[k][0], 4), member_share=round(facts[k][1], 4), rel_l2_vs_float64=float("%.3g" % facts[k][2]),
                                  underflowed_pixels_left_out=facts[k][3])
                        e["over_floor"] = round(e["ms"] / e["floor_ms"], 3)
                        # how far the launch is behind the pre-pass's distance from its floor, in spreads of the two
                        e["behind_prepass_ratio_in_spreads"] = round((e["ms"] - pre["over_floor"] * e["floor_ms"]) / max(e["spread_ms"], pre["spread_ms"], 1e-6), 2)
                        lines.append(e)
                    del keep, cands
                # ---- the preview path against the full filter
                if "preview" not in skip:
                    for radius in (20, 6):
                        fs.radius = radius
                        fs._previews.clear()
                        # every step with its argument blocks built once: the calls below only enqueue
                        full_args, keep_full = fs.filter_args()
                        cands, keep = {"filter_f32x3": (lambda: api.filter_f32x3(full_args))}, []
                        for k in KS:
                            want = fs.preview(k).clone()       # allocates the coarse film of this k
                            coarse = fs._previews[k]
                            es, _ = fs._pool_entries(coarse)
                            fa, keep_f = fs.filter_args()
                            ca, keep_c = coarse.filter_args()
                            keep.append((es, fa, ca, keep_f, keep_c))

                            def steps(es=es, fa=fa, ca=ca, k=k):
                                api.pool_statistics(W, H, k, es)       # its epilogue is the coarse pre-pass
                                api.window_filter(ca, 3)
                                api.upsample_filtered(fa, ca, k, 3)     # the fine pre-pass is the accumulation's epilogue
                            fs.film_f.zero_()
                            steps()
                            if not torch.equal(fs.film_f.view(torch.int32), want.view(torch.int32)):
                                sys.exit("time_upsample.py: the timed steps do not leave FilmStats.preview(%d)'s bits at %d x %d" % (k, W, H))
                            cands["preview_k%d" % k] = steps
                        runs = rounds(cands)
                        full = entry("filter_f32x3", W, H, runs, radius=radius)
                        lines.append(full)
                        for k in KS:
                            e = entry("preview_k%d" % k, W, H, runs, radius=radius)
                            e["ratio_to_filter"] = round(e["ms"] / full["ms"], 4)
                            e["ahead_in_spreads"] = round((full["ms"] - e["ms"]) / max(e["spread_ms"], full["spread_ms"], 1e-6), 1)
                            lines.append(e)
                    fs.radius = 20
                del fs, scene
                torch.cuda.empty_cache()
            # ---- quality: what a preview gives up
            if "quality" not in skip:
                W, H = 960, 540
                scene = synthetic.Scene(W, H, n_regions=12, seed=1, device=dev)
                truth = scene.truth * FIREFLY
                fs = film.FilmStats(W, H, dev, fused_prepass=True)
                done = 0
                for spp in (4, 16, 64):
                    while done < spp:
                        s = min(8, spp - done)
                        fs.accumulate(scene.samples(s, seed=100 + done, features=("radiance", "normal", "albedo")))
                        done += s
                    q = {"kernel": "quality", "width": W, "height": H, "spp": spp, "reference": "the scene's expectation",
                         "noisy": rel_l2(fs.state["radiance"]["film_mean"], truth), "filter_f32x3": rel_l2(fs.denoise(), truth)}
                    for k in (2, 4):
                        q["preview_k%d" % k] = rel_l2(fs.preview(k), truth)
                    lines.append({key: (round(v, 5) if isinstance(v, float) else v) for key, v in q.items()})
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_stream_destroy(handle))
    lines = [json.dumps(line) for line in lines]
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
