"""Times statmc_error_scores and statmc_plan_to_target at 1920 x 1080 and 3840 x 2160, in one process, against the library's own
launches of comparable traffic:

  error_scores    3 channels, relative metric; without a table (the standard error) and with table 0 (the built-in two-sided
                  quantiles); n uniform (8 everywhere: every lane gathers the same entry) and n drawn per pixel from 2..4097 (every
                  degree of freedom of the table, neighbours at unrelated entries: the worst case for the gather)
  sample_scores   statmc_sample_scores on the same planes: the yardstick, the same 32 B/px without the division by n and the gather;
                  every error_scores line carries its ratio to the sample_scores line of the same n
  plan_to_target  on the error image of the per-pixel n, targets at the image's median (half the film open) and at its 99th
                  percentile; 12 B/px
  count_above     statmc_score_count_above with one threshold on the same image: the yardstick, a one-pass reduction of 4 B/px
  floor           the bytes of each launch at the copy bandwidth measured in the same process (a device-to-device copy of 512 MiB:
                  bytes read plus bytes written over its time)

Refuses to report unless the device's bits equal the numpy restatement's (tests/error_reference.py) for every timed configuration
(NaN excepted as in the tests: none occurs here).  Everything runs on one library stream (statmc_stream_create), events recorded on
it.  One JSON line per (size, candidate): milliseconds per call (50 calls after 10, five alternating rounds: every round times every
candidate once; mean over the rounds, and the runs), spread = max - min over the rounds.

    python tools/time_error_scores.py [--iters 50 --warmup 10 --rounds 5] [--out profiles/error_scores.jsonl]
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
import error_reference as ref  # noqa: E402
import plan_reference as plan  # noqa: E402
from statmc_amd import api  # noqa: E402

SIZES = ((1920, 1080), (3840, 2160))
TABLE = 0
C_MIN, C_MAX = 1, 64


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


def device_table(lib, table):
    """the 4096 quantiles of the built-in table: what statmc_set_t_quantiles(table, NULL, 0) leaves on the device, read from the
    header the library is built from"""
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "statmc_amd", "csrc", "t_quantiles.h")).read(), flags=re.S)
    rows = re.findall(r"\{([^{}]*)\}", text[text.index("statmc_tq_tables"):])
    rows = [np.array([float(v.rstrip("fF")) for v in r.replace("\n", " ").split(",") if v.strip()], np.float32) for r in rows]
    rows = [r for r in rows if r.size == 4096]
    if len(rows) != 6:
        sys.exit("time_error_scores.py: cannot read the six tables of t_quantiles.h")
    return rows[table]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_error_scores.py measures on the GPU: no device")
    dev = torch.device("cuda:0")
    api.setup(0)
    lib = api.load()
    api.check(lib.statmc_set_t_quantiles(TABLE, None, 0))
    tq = device_table(lib, TABLE)
    handle = C.c_void_p()
    api.check(lib.statmc_stream_create(C.byref(handle)))
    stream = torch.cuda.ExternalStream(handle.value, device=dev)
    lines = []
    try:
        with torch.cuda.stream(stream):      # api.* and torch both enqueue on the library stream
            src = torch.empty(512 << 20, dtype=torch.uint8, device=dev).fill_(1)
            dst = torch.empty_like(src)
            bw = 2 * src.numel() / (timed(lambda: dst.copy_(src), 20, 3, stream) * 1e-3)
            del src, dst
            lines.append(json.dumps({"kernel": "copy_512MiB", "tb_per_s": round(bw / 1e12, 3)}))
            for W, H in SIZES:
                px = W * H
                rng = np.random.default_rng(W)
                h_n = {"uniform": np.full((H, W), 8, np.int32), "per_pixel": rng.integers(2, 4098, (H, W)).astype(np.int32)}
                h_mean = rng.random((H, W, 3), dtype=np.float32)
                h_m2 = (rng.random((H, W, 3), dtype=np.float32) * h_n["per_pixel"][..., None]).astype(np.float32)
                n = {k: torch.from_numpy(v).to(dev) for k, v in h_n.items()}
                mean, m2 = torch.from_numpy(h_mean).to(dev), torch.from_numpy(h_m2).to(dev)
                out = torch.empty((H, W), dtype=torch.float32, device=dev)
                counts = torch.empty((H, W), dtype=torch.int32, device=dev)
                result = torch.empty(6, dtype=torch.int64, device=dev)
                above = torch.empty(1, dtype=torch.int64, device=dev)
                # the device's bits against the restatement's, every configuration that is timed
                errors = None
                for kind in n:
                    for table, quantiles in (("none", None), ("table", tq)):
                        want = ref.error_scores_ref(h_n[kind], h_mean, h_m2, plan.RELATIVE, 1e-3, quantiles)
                        got = api.error_scores(n[kind], mean, m2, table=api.ERROR_NO_TABLE if quantiles is None else TABLE).cpu().numpy()
                        if np.isnan(want).any() or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                            sys.exit("time_error_scores.py: the device's error scores differ from the restatement's at %d x %d (%s, %s)" % (W, H, kind, table))
                        if kind == "per_pixel" and quantiles is not None:
                            errors = want
                d_errors = torch.from_numpy(errors).to(dev)
                flat = np.sort(errors.reshape(-1))
                targets = {"median": float(flat[px // 2]), "p99": float(flat[int(px * 0.99)])}
                for name, t in targets.items():
                    want, want_res = ref.plan_to_target_ref(errors, h_n["per_pixel"], t, C_MIN, C_MAX)
                    got, res = api.plan_to_target(d_errors, n["per_pixel"], t, C_MIN, C_MAX, out=counts, result=result, return_result=True)
                    if not np.array_equal(got.cpu().numpy(), want) or {k: res[k] for k in want_res} != want_res:
                        sys.exit("time_error_scores.py: the device's plan to the target differs from the restatement's at %d x %d (%s)" % (W, H, name))
                cands = {}
                for kind in n:
                    cands["sample_scores_n_%s" % kind] = (lambda kind=kind: api.sample_scores(n[kind], mean, m2, out=out))
                    cands["error_scores_none_n_%s" % kind] = (lambda kind=kind: api.error_scores(n[kind], mean, m2, table=api.ERROR_NO_TABLE, out=out))
                    cands["error_scores_table_n_%s" % kind] = (lambda kind=kind: api.error_scores(n[kind], mean, m2, table=TABLE, out=out))
                for name, t in targets.items():
                    cands["plan_to_target_%s" % name] = (lambda t=t: api.plan_to_target(d_errors, n["per_pixel"], t, C_MIN, C_MAX, out=counts, result=result))
                    cands["count_above_%s" % name] = (lambda t=t: api.score_count_above(d_errors, [t], out=above))
                runs = {name: [] for name in cands}
                for rnd in range(a.rounds):                  # alternating: every round times every candidate once
                    for name, fn in cands.items():
                        runs[name].append(timed(fn, a.iters, a.warmup if rnd == 0 else 3, stream))
                avg = {name: sum(v) / len(v) for name, v in runs.items()}
                spread = {name: max(v) - min(v) for name, v in runs.items()}
                for name in cands:
                    ms = avg[name]
                    line = {"kernel": name, "width": W, "height": H, "ms": round(ms, 4), "runs_ms": [round(x, 4) for x in runs[name]],
                            "spread_ms": round(spread[name], 4), "same_bits_as_restatement": True}
                    if name.startswith(("error_scores", "sample_scores")):
                        line["floor_ms"] = round(32 * px / bw * 1e3, 4)
                    if name.startswith("error_scores"):
                        kind = name.split("_n_")[1]
                        line["ratio_to_sample_scores"] = round(ms / avg["sample_scores_n_%s" % kind], 3)
                    if name.startswith("error_scores_table"):
                        other = name.replace("_table_", "_none_")
                        line["ms_over_no_table"] = round(ms - avg[other], 4)
                        line["behind_no_table_in_spreads"] = round((ms - avg[other]) / max(spread[name], spread[other], 1e-6), 2)
                    if name.startswith("plan_to_target"):
                        line["floor_ms"] = round(12 * px / bw * 1e3, 4)
                        line["ratio_to_count_above"] = round(ms / avg[name.replace("plan_to_target", "count_above")], 3)
                    if name.startswith("count_above"):
                        line["floor_ms"] = round(4 * px / bw * 1e3, 4)
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
