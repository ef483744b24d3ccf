"""Times statmc_compact_accumulate_interleaved -- the compact (CSR) arena as ONE array of interleaved records, pixel p's records at
slots [offsets[p], offsets[p + 1]) -- against what a renderer could call instead, at 1920 x 1080 with the five stat types of
film.STAT_TYPES (11 channels), records and moments from statmc_malloc_placed.  One process per set, every layout in it:

    python tools/time_accumulate_compact_interleaved.py --set a|b|c|d [--out profiles/accumulate_compact_interleaved.jsonl
                                                                       --iters 30 --warmup 5 --rounds 5 --windows 12288,24576,65536]

  a  16 samples on every pixel.                     c  one per pixel plus 16 pixels at 65 536 (split_above = 256).
  b  every pixel its own count, uniform in 1 .. 64. d  5 % of the pixels at 256 samples, the others at none.
(the four data sets of DESIGN.md 4.1j, tools/time_accumulate_compact.py's count maps.)

Layouts: tight44 -- {radiance, normal, albedo, depth, id} fp32 back to back; padded48 -- the same with 4 bytes of padding;
half28 -- radiance fp32, the four feature fields IEEE half.  The yardsticks are timed again in this process:
  compact       statmc_compact_accumulate on the de-interleaved arenas, each in its field's format, default dispatch
  records_ilv   statmc_accumulate_records_interleaved (set c: _split at 256) on records of the same fields that carry their owner
                in a pixel field: padded48's own records with the owner in the padding; for tight44 and half28 records 4 bytes
                longer with the owner behind the fields.
Before anything is timed every path of the new entry -- default dispatch, fused staged at the default window and at every window of
--windows, fused direct, general -- and records_ilv run once from zeroed moments and every state image is compared with the
compact yardstick's (`bits_equal`).  Then `rounds` rounds time every entry alternately in this one process, `iters` calls after
`warmup` each (hipEvent timing, moments zeroed before each series); mean over the rounds, spread = max - min.  "Ahead" means beyond
3 x the larger spread.

Per set and layout one JSON line (appended to --out as well): the ms of each entry, its spread, the share of the waves that stage
under each window, and the byte model -- stride * total + 16 B per pixel of offsets + 2 x the state bytes of the touched pixels --
over the default call's time as a share of the 8 TB/s HBM peak."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from statmc_amd import api, film  # noqa: E402
from time_accumulate_compact import FIELDS, INT32_MAX, PEAK, TYPES, count_map, state_bytes_per_pixel, timed  # noqa: E402

# kCompactIlvWindowDefault of statmc_compact_interleaved_args.h, restated by hand: the library has no getter for it, so
# `default_window` and the key of `staged_wave_share` follow this line, not the header -- change both together
DEFAULT_WINDOW = 49 * 1024
F32, F16 = api.SAMPLES_F32, api.SAMPLES_F16
# name -> (stride, byte offset per type of TYPES, format per type)
LAYOUTS = {
    "tight44": (44, (0, 12, 24, 36, 40), (F32,) * 5),
    "padded48": (48, (0, 12, 24, 36, 40), (F32,) * 5),
    "half28": (28, (0, 12, 18, 24, 26), (F32, F16, F16, F16, F16)),
}


def interleave(arenas, stride, offs, fmts, dev, owners=None, pixel_offset=None):
    """[total, stride] uint8 from placed memory: field t of record i = arenas[t][i] in its format; owners at pixel_offset."""
    total = arenas[0].shape[0]
    rec = api.empty_placed((total, stride), torch.uint8, dev, api.MEM_STREAM)
    rec.fill_(0xEE)
    r32, r16 = rec.view(torch.int32), rec.view(torch.int16)
    for a, o, f in zip(arenas, offs, fmts):
        c = a.shape[1]
        if f == F16:
            r16[:, o // 2:o // 2 + c] = a.view(torch.int16)
        else:
            r32[:, o // 4:o // 4 + c] = a.view(torch.int32)
    if owners is not None:
        r32[:, pixel_offset // 4] = owners
    return rec


def staged_wave_share(offsets, counts, base, stride, window, split_above):
    """The share of the waves with records that the staged kernel stages, by the kernel's own rule restated on the offsets: the span
    of the wave's 64 pixels, from the 16-byte boundary below its first byte, fits the window and no run in it is above split_above."""
    npx = counts.numel()
    edges = torch.arange(0, npx + 64, 64, device=offsets.device).clamp_(max=npx)
    first, last = offsets[edges[:-1]], offsets[edges[1:]]
    span = (base + first * stride) % 16 + (last - first) * stride
    longest = torch.nn.functional.pad(counts.view(-1), (0, -npx % 64)).view(-1, 64).max(dim=1).values
    live = last > first
    return round(float(((span <= window) & (longest <= split_above) & live).sum()) / max(int(live.sum()), 1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=("a", "b", "c", "d"), required=True)
    ap.add_argument("--layouts", default="tight44,padded48,half28")
    ap.add_argument("--windows", default="12288,24576,65536", help="LDS windows of the staged kernel timed next to the default one")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    W, H = a.width, a.height
    npx = W * H
    dev = torch.device("cuda:0")
    api.setup(0)
    cfg = film.STAT_TYPES
    ch = [cfg[t]["channels"] for t in TYPES]
    stream = api.current_stream_handle()
    windows = [int(w) for w in a.windows.split(",") if w]

    counts = count_map(a.set, W, H, dev)
    total = int(counts.sum())
    touched = int((counts > 0).sum())
    offsets, owners = api.compact_offsets(counts, owners_capacity=total)
    torch.cuda.synchronize()
    assert int(offsets[-1]) == total
    split = 256 if a.set == "c" else INT32_MAX

    gen = torch.Generator(device=dev).manual_seed(11)
    values = [torch.rand((total, c), device=dev, generator=gen).square_().add_(0.01) for c in ch]
    fs = film.FilmStats(W, H, dev, types=TYPES, placed=True)
    field_types = [api.make_stat_type_record_field(c, fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for t, c in zip(TYPES, ch)]

    def images():
        return [fs.state[t][k] for t in TYPES for k in FIELDS if fs.state[t].get(k) is not None]

    for name in a.layouts.split(","):
        stride, offs, fmts = LAYOUTS[name]
        api.placement_expect(api.MEM_STREAM, total * (2 * stride + 4 + 44), dev)
        arenas = []
        for v, c, f in zip(values, ch, fmts):
            arena = api.empty_placed((total, c), torch.float16 if f == F16 else torch.float32, dev, api.MEM_STREAM)
            arena.copy_(v)
            arenas.append(arena)
        rec = interleave(arenas, stride, offs, fmts, dev, owners=owners if stride == 48 else None, pixel_offset=44)
        rec_owned, owned_stride = (rec, 48) if stride == 48 else (interleave(arenas, stride + 4, offs, fmts, dev, owners=owners, pixel_offset=stride), stride + 4)
        api.placement_expect(api.MEM_STREAM, 0, dev)
        layout = api.make_record_layout(stride, 0, offs, fmts)
        owned_layout = api.make_record_layout(owned_stride, 44 if stride == 48 else stride, offs, fmts)
        compact_types = [api.make_stat_type_compact(arenas[i], ch[i], fs.state[t], cfg[t]["transform"], cfg[t]["max_moment"]) for i, t in enumerate(TYPES)]
        formats = list(fmts) if F16 in fmts else None

        # the dispatch of an entry's series is pinned once, outside the timed region (run_series): what is timed is the call alone
        pinned = {}

        def ilv(path, window=0):
            def call():
                api.compact_accumulate_interleaved(W, H, field_types, rec, layout, offsets, n_records=total, split_above=split, stream=stream)
            pinned[call] = (path, window)
            return call

        def run_series(fn, series):
            path, window = pinned.get(fn, (api.COMPACT_ILV_PATH_AUTO, 0))
            api.compact_interleaved_path(path)
            api.compact_interleaved_window(window)
            try:
                return series(fn)
            finally:
                api.compact_interleaved_path(api.COMPACT_ILV_PATH_AUTO)
                api.compact_interleaved_window(0)

        runs = {"ilv": ilv(api.COMPACT_ILV_PATH_AUTO), "ilv_staged": ilv(api.COMPACT_ILV_PATH_FUSED_STAGED), "ilv_direct": ilv(api.COMPACT_ILV_PATH_FUSED_DIRECT),
                "ilv_general": ilv(api.COMPACT_ILV_PATH_GENERAL)}
        for w in windows:
            runs["ilv_staged_w%d" % w] = ilv(api.COMPACT_ILV_PATH_FUSED_STAGED, w)
        runs["compact"] = lambda: api.compact_accumulate(W, H, compact_types, offsets, n_samples=total, sample_formats=formats, split_above=split, stream=stream)
        runs["records_ilv"] = lambda: api.accumulate_records_interleaved(W, H, field_types, rec_owned, owned_layout, n_records=total, stream=stream,
                                                                         split_above=256 if a.set == "c" else None)

        # ---- the same bits as the compact entry on the de-interleaved arenas, on every path
        fs.reset()
        runs["compact"]()
        want = [img.clone() for img in images()]
        equal, default_path, differs = True, 0, []
        for k in runs:
            if k == "compact":
                continue
            fs.reset()
            run_series(runs[k], lambda fn: fn())
            if k == "ilv":
                default_path = api.last_compact_interleaved_path()
            ok = all(torch.equal(g.view(torch.int32), img.view(torch.int32)) for g, img in zip(want, images()))
            equal = equal and ok
            if not ok:
                differs.append(k)
        del want
        if not equal:
            print(json.dumps({"set": a.set, "layout": name, "bits_equal": False, "differs": differs}), flush=True)
            sys.exit(1)

        # ---- timings, alternating
        ms = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                fs.reset()
                ms[k].append(run_series(fn, lambda f: timed(f, a.iters, a.warmup)))
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        model_bytes = stride * total + 16 * npx + 2 * state_bytes_per_pixel() * touched
        out = {"set": a.set, "layout": name, "stride": stride, "width": W, "height": H, "channels": sum(ch), "total_records": total,
               "mean_count": round(total / npx, 3), "touched_pixels": touched, "split_above": split, "iters": a.iters, "warmup": a.warmup,
               "rounds": a.rounds, "placed": api.placement_info()["active"] == 1, "default_path": default_path, "default_window": DEFAULT_WINDOW,
               "bits_equal": True, "model_bytes": model_bytes, "ilv_of_peak": round(model_bytes / (mean["ilv"] * 1e-3) / PEAK, 4)}
        out["staged_wave_share"] = {str(w): staged_wave_share(offsets, counts, rec.data_ptr(), stride, w, split) for w in [DEFAULT_WINDOW] + windows}
        for k in runs:
            out[k + "_ms"] = round(mean[k], 4)
            out[k + "_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
            out[k + "_runs_ms"] = [round(v, 4) for v in ms[k]]
        out["staged_over_direct"] = round(mean["ilv_staged"] / mean["ilv_direct"], 3)
        out["ilv_over_compact"] = round(mean["ilv"] / mean["compact"], 3)
        out["ilv_over_records_ilv"] = round(mean["ilv"] / mean["records_ilv"], 3)
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del arenas, rec, rec_owned, compact_types, runs, pinned
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
