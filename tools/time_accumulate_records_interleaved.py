"""Times statmc_accumulate_records_interleaved -- the queue of finished samples as one interleaved record per sample -- against
statmc_accumulate_records on the same samples de-interleaved into one array per stat type, in ONE process, at 1920 x 1080 with
the five stat types of film.STAT_TYPES (11 channels) and moments from statmc_malloc_placed.  The record sets are those of
tools/time_accumulate_records.py:

    python tools/time_accumulate_records_interleaved.py --set a|b|c [--width 1920 --height 1080 --iters 50 --warmup 10]

  a  16 records for every pixel; the records of sample s visit the pixels in a shuffled order of their own
  b  the same records in film order: record s * W * H + p belongs to pixel p
  c  sparse: 5 % of the pixels at 256 records each, the pixels of sample s in a shuffled order of their own

Four inputs, the same records in each:
  arrays   pixels[] + five fp32 arrays, statmc_accumulate_records: the yardstick, code this entry does not touch
  rec48    {pixel, radiance, normal, albedo, depth, id}, every field fp32: 48 B
  rec32    the radiance fp32, the four feature fields in IEEE half: 4 + 12 + 16 = 32 B (28 B of samples behind the pixel index)
  rec28    every field half: 4 + 22 = 26 B, padded to 28 (the radiance clamped to half's range first)
Per input: the whole call, its grouping step and its fold alone (statmc_debug_accumulate_records_phases), each timed five times with
hipEvents, `iters` calls after `warmup`: the mean, and max - min as the spread.  The interleaved inputs also have the fold through
the general kernel (statmc_debug_accumulate_records_interleaved_path(1)); `fold_ms` is the library's own choice, the fused kernel.
`bits_equal`: before anything is timed, each interleaved input and the arrays entry on the same values (half fields widened to
fp32) run once from zeroed moments and every state image is compared bitwise.  One JSON line per set.

Byte model of the fold: stride + 8 bytes per record (the record and its order[] entry, read once), plus the
state of the touched pixels read and written; for the arrays 4 * 11 + 8 per record (the fold does not read pixels[])."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402

PEAK = 8.0e12
TYPES = ("radiance", "normal", "albedo", "depth", "materialid")
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
REPEATS = 5


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
    cfg = film.STAT_TYPES
    ch = {t: cfg[t]["channels"] for t in TYPES}
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = api.current_stream_handle()
    lib = api.load()

    # ---- the record set: pixels[] and, per type, [n_rec, C] fp32 values (radiance log-normal and clamped to half's range, so
    # that all inputs hold the same records; features in [0, 1))
    if a.set == "b":
        pixels = torch.arange(npx, dtype=torch.int32, device=dev).repeat(S)
        n_touched = npx
    else:
        subset = torch.arange(npx, device=dev) if a.set == "a" else torch.randperm(npx, device=dev, generator=gen)[:npx // 20]
        pixels = torch.cat([subset[torch.randperm(subset.numel(), device=dev, generator=gen)] for _ in range(S)]).to(torch.int32).contiguous()
        n_touched = subset.numel()
    n_rec = pixels.numel()
    values = {}
    for t in TYPES:
        if t == "radiance":
            values[t] = torch.randn(n_rec, 3, device=dev, generator=gen).exp_().clamp_(max=60000.0)
        else:
            values[t] = torch.rand(n_rec, ch[t], device=dev, generator=gen)
    half = {t: values[t].to(torch.float16) for t in TYPES}
    px_col = pixels.view(-1, 1)
    as_i32 = lambda x: x.contiguous().view(torch.int32)
    feats16 = torch.cat([half[t] for t in TYPES[1:]], 1)                                           # [n, 8] half
    all16 = torch.cat([half[t] for t in TYPES] + [torch.zeros(n_rec, 1, dtype=torch.float16, device=dev)], 1)   # [n, 12] half, the last one padding
    inputs = {
        "rec48": dict(records=placed_copy(torch.cat([px_col] + [as_i32(values[t]) for t in TYPES], 1), dev),
                      layout=api.make_record_layout(48, 0, [4, 16, 28, 40, 44]), widen=()),
        "rec32": dict(records=placed_copy(torch.cat([px_col, as_i32(values["radiance"]), as_i32(feats16)], 1), dev),
                      layout=api.make_record_layout(32, 0, [4, 16, 22, 28, 30], [api.SAMPLES_F32] + [api.SAMPLES_F16] * 4), widen=TYPES[1:]),
        "rec28": dict(records=placed_copy(torch.cat([px_col, as_i32(all16)], 1), dev),
                      layout=api.make_record_layout(28, 0, [4, 10, 16, 22, 24], [api.SAMPLES_F16] * 5), widen=TYPES),
    }
    del feats16, all16
    for name, inp in inputs.items():
        assert inp["records"].shape == (n_rec, inp["layout"].stride // 4), name
    arrays = {t: placed_copy(values[t], dev) for t in TYPES}
    pixels = placed_copy(pixels, dev)
    del values

    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    field_types = [api.make_stat_type_record_field(ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    def array_types(src):
        return [api.make_stat_type_records(src[t], ch[t], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t in TYPES]

    def images():
        return [fs.state[t][k] for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    def phases(p):
        api.check(lib.statmc_debug_accumulate_records_phases(p))

    # ---- the same bits as the arrays entry on the same values
    bits_equal, path_taken = {}, {}
    for name, inp in inputs.items():
        src = {t: (half[t].to(torch.float32) if t in inp["widen"] else arrays[t]) for t in TYPES}
        fs.reset()
        api.accumulate_records(W, H, array_types(src), pixels, stream=stream)
        want = [img.clone().view(torch.int32) for img in images()]
        del src
        equal = True
        for path in (api.RECORDS_PATH_AUTO, api.RECORDS_PATH_GENERAL):
            fs.reset()
            api.accumulate_records_interleaved_path(path)
            api.accumulate_records_interleaved(W, H, field_types, inp["records"], inp["layout"], stream=stream)
            api.accumulate_records_interleaved_path(api.RECORDS_PATH_AUTO)
            if path == api.RECORDS_PATH_AUTO:
                path_taken[name] = api.last_accumulate_records_interleaved_path()
            equal = equal and all(torch.equal(w, img.view(torch.int32)) for w, img in zip(want, images()))
        bits_equal[name] = bool(equal)
        del want
    del half

    # ---- timings; the moments are zeroed before each series, so counts stay far below 2^24
    def series(fn, phase):
        out = []
        for _ in range(REPEATS):
            if phase == 2:                    # the fold alone runs over the index a grouping-only call of the same input leaves
                phases(1)
                fn()
            phases(phase)
            fs.reset()
            out.append(timed(fn, a.iters, a.warmup))
        phases(3)
        return {"ms": round(sum(out) / len(out), 4), "spread_ms": round(max(out) - min(out), 4), "runs_ms": [round(v, 4) for v in out]}

    state_b = 2 * state_bytes_per_pixel()
    share = lambda b, ms: round(b / (ms * 1e-3) / PEAK, 4)
    result = {"set": a.set, "width": W, "height": H, "records": n_rec, "records_per_touched_pixel": S, "touched_pixels": n_touched,
              "iters": a.iters, "warmup": a.warmup, "repeats": REPEATS, "placed": api.placement_info()["active"] == 1,
              "bits_equal": bits_equal, "path_taken": path_taken}

    types_arrays = array_types(arrays)
    run_arrays = lambda: api.accumulate_records(W, H, types_arrays, pixels, stream=stream)
    r = {"call": series(run_arrays, 3), "grouping": series(run_arrays, 1), "fold": series(run_arrays, 2)}
    r["fold_bytes"] = n_rec * (4 * 11 + 8) + n_touched * state_b
    r["fold_of_peak"] = share(r["fold_bytes"], r["fold"]["ms"])
    result["arrays"] = r
    for name, inp in inputs.items():
        run = lambda inp=inp: api.accumulate_records_interleaved(W, H, field_types, inp["records"], inp["layout"], stream=stream)
        r = {"stride": inp["layout"].stride, "call": series(run, 3), "grouping": series(run, 1), "fold": series(run, 2)}
        api.accumulate_records_interleaved_path(api.RECORDS_PATH_GENERAL)
        r["fold_general"] = series(run, 2)
        api.accumulate_records_interleaved_path(api.RECORDS_PATH_AUTO)
        r["fold_bytes"] = n_rec * (inp["layout"].stride + 8) + n_touched * state_b
        r["fold_of_peak"] = share(r["fold_bytes"], r["fold"]["ms"])
        # what has to hold on the shuffled sets: the interleaved fold beats the per-array fold by more than 3 x the larger spread
        gain = result["arrays"]["fold"]["ms"] - r["fold"]["ms"]
        r["fold_gain_ms"] = round(gain, 4)
        r["fold_gain_over_3_spreads"] = bool(gain > 3 * max(result["arrays"]["fold"]["spread_ms"], r["fold"]["spread_ms"]))
        r["arrays_fold_over_fold"] = round(result["arrays"]["fold"]["ms"] / r["fold"]["ms"], 3)
        result[name] = r
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
