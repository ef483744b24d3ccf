"""statmc_error_scores / statmc_plan_to_target (include/statmc.h) without a GPU: the symbols, their declarations and the ctypes
mirrors; the argument checks of statmc_amd/csrc/statmc_error_args.h -- compiled alone into tests/cpp/test_error_args.cpp, plain and
under AddressSanitizer and UBSan -- against a Python restatement of the header's rules, in the header's order; what the built library
answers without a device; and the properties of the numpy float32 restatement (tests/error_reference.py) that
tests/test_error_scores_gpu.py holds the device to -- among them the fact the entries exist for: the error of the mean falls as
samples arrive, the sample deviation does not."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import error_reference as ref
import plan_reference as plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_error_args.cpp")
F32 = np.float32
FW, FH = 64, 48
MIB = 1 << 20
N_AT, MEAN_AT, M2_AT, SCORE_AT, COUNTS_AT, RESULT_AT = (i * 16 * MIB for i in range(1, 7))   # made-up images, 16 MiB apart
PX = FW * FH * 4
CHUNK, MAX_GRID = 1024, 1024      # pixels per workgroup and step; workgroups of the plan's one pass


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- the table of calls and the restatement of include/statmc.h
def error(**kw):
    c = dict(kind="error", width=FW, height=FH, channels=3, metric=1, eps=1e-3, table=-1, n=N_AT, film_mean=MEAN_AT, film_m2=M2_AT, score=SCORE_AT)
    c.update(kw)
    return c


def target(**kw):
    c = dict(kind="target", width=FW, height=FH, target=0.02, c_min=1, c_max=32, error=SCORE_AT, n=N_AT, sample_counts=COUNTS_AT, result=RESULT_AT)
    c.update(kw)
    return c


def table():
    t = {}
    t["valid_error"] = error()
    for k in range(6):
        t["valid_error_table_%d" % k] = error(table=k)
    t["valid_error_one_channel_absolute"] = error(channels=1, metric=0, table=5)
    t["valid_error_absolute_ignores_eps"] = error(metric=0, eps=-1.0)
    t["valid_error_unaligned_plane"] = error(film_m2=M2_AT + 4)
    t["valid_error_odd_film"] = error(width=37, height=29)
    t["valid_error_score_right_behind_n"] = error(score=N_AT + PX)
    t["error_zero_width"] = error(width=0)
    t["error_zero_height"] = error(height=0)
    t["error_channels_2"] = error(channels=2)
    t["error_metric_2"] = error(metric=2)
    t["error_metric_minus_1"] = error(metric=-1)
    t["error_table_6"] = error(table=6)
    t["error_table_minus_2"] = error(table=-2)
    t["error_metric_comes_before_table"] = error(metric=2, table=9)
    t["error_table_comes_before_eps"] = error(table=6, eps=0.0)
    t["error_eps_comes_before_null"] = error(eps=0.0, n=0)
    for name, eps in (("zero", 0.0), ("negative", -1e-3), ("inf", float("inf")), ("nan", float("nan"))):
        t["error_eps_" + name] = error(eps=eps)
    for p in ("n", "film_mean", "film_m2", "score"):
        t["error_null_" + p] = error(**{p: 0})
        t["error_misaligned_" + p] = error(**{p: error()[p] + 2})
    t["error_score_is_n"] = error(score=N_AT)
    t["error_score_in_the_last_bytes_of_n"] = error(score=N_AT + PX - 4)
    t["error_score_in_the_last_bytes_of_film_mean"] = error(score=MEAN_AT + 3 * PX - 4)
    t["valid_error_score_right_behind_film_mean"] = error(score=MEAN_AT + 3 * PX)
    t["error_score_ends_inside_film_m2"] = error(score=M2_AT - PX + 4)

    t["valid_target"] = target()
    t["valid_target_odd_film"] = target(width=37, height=29)
    t["valid_target_unaligned_counts"] = target(sample_counts=COUNTS_AT + 4)
    t["valid_target_zero_counts"] = target(c_min=0, c_max=0)
    t["valid_target_largest_c_max"] = target(c_min=0, c_max=1 << 20)
    t["valid_target_smallest_target"] = target(target=2.0 ** -60)
    t["valid_target_largest_target"] = target(target=2.0 ** 60)
    far = dict(error=1 << 40, n=2 << 40, sample_counts=3 << 40, result=4 << 40)    # images of up to 16 GiB
    t["valid_target_4k_film"] = target(width=3840, height=2160, **far)
    t["valid_target_largest_film"] = target(width=65535, height=65535, c_max=1 << 20, **far)
    t["target_zero_width"] = target(width=0)
    t["target_zero_height"] = target(height=0)
    for p in ("error", "n", "sample_counts", "result"):
        t["target_null_" + p] = target(**{p: 0})
    for p in ("error", "n", "sample_counts"):
        t["target_misaligned_" + p] = target(**{p: target()[p] + 2})
    t["target_misaligned_result"] = target(result=RESULT_AT + 4)
    for name, v in (("zero", 0.0), ("negative", -0.02), ("nan", float("nan")), ("inf", float("inf")), ("below_the_live_class", 2.0 ** -61),
                    ("above_the_live_class", float(np.nextafter(F32(2.0 ** 60), F32(np.inf))))):
        t["target_target_" + name] = target(target=v)
    t["target_alignment_comes_before_the_target"] = target(target=0.0, n=N_AT + 2)
    t["target_the_target_comes_before_the_bounds"] = target(target=0.0, c_min=-1)
    t["target_negative_c_min"] = target(c_min=-1)
    t["target_c_min_above_c_max"] = target(c_min=9, c_max=8)
    t["target_c_max_above_the_limit"] = target(c_max=(1 << 20) + 1)
    t["target_counts_is_error"] = target(sample_counts=SCORE_AT)
    t["target_counts_is_n"] = target(sample_counts=N_AT)
    t["target_counts_in_the_last_bytes_of_error"] = target(sample_counts=SCORE_AT + PX - 4)
    t["valid_target_counts_right_behind_error"] = target(sample_counts=SCORE_AT + PX)
    t["target_counts_end_inside_n"] = target(sample_counts=N_AT - PX + 4)
    t["valid_target_counts_end_at_n"] = target(sample_counts=N_AT - PX)
    t["target_counts_over_result"] = target(result=COUNTS_AT + 8)
    t["target_counts_over_the_last_bytes_of_result"] = target(sample_counts=RESULT_AT + 40)
    t["valid_target_counts_right_behind_result"] = target(sample_counts=RESULT_AT + 48)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def restated(c):
    """include/statmc.h's error lists, in their order: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    px = c["width"] * c["height"] * 4
    if c["kind"] == "error":
        if c["channels"] not in (1, 3):
            return ["channels"]
        if c["metric"] not in (0, 1):
            return ["metric"]
        if not -1 <= c["table"] <= 5:
            return ["table"]
        if c["metric"] == 1 and not (c["eps"] > 0 and np.isfinite(c["eps"])):
            return ["eps"]
        for p in ("n", "film_mean", "film_m2", "score"):
            if c[p] == 0:
                return ["null " + p]
        for p in ("n", "film_mean", "film_m2", "score"):
            if c[p] % 4:
                return [p, "aligned"]
        for p, nb in (("n", px), ("film_mean", px * c["channels"]), ("film_m2", px * c["channels"])):
            if overlap(c["score"], px, c[p], nb):
                return ["score overlaps " + p]
        return None
    for p in ("error", "n", "sample_counts", "result"):
        if c[p] == 0:
            return ["null " + p]
    for p, a in (("error", 4), ("n", 4), ("sample_counts", 4), ("result", 8)):
        if c[p] % a:
            return [p, "aligned"]
    tf = F32(c["target"])
    if not (tf >= F32(2.0 ** -60) and tf <= F32(2.0 ** 60)):
        return ["target"]
    if not 0 <= c["c_min"] <= c["c_max"] <= 1 << 20:
        return ["c_min", "c_max"]
    for p, nb in (("error", px), ("n", px), ("result", 48)):
        if overlap(c["sample_counts"], px, c[p], nb):
            return ["sample_counts overlaps " + p]
    return None


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def write_table(path, calls):
    with open(path, "w") as f:
        for name, c in calls.items():
            if c["kind"] == "error":
                f.write("error %s %d %d %d %d %d %d %d %d %d %d\n" % (name, c["width"], c["height"], c["channels"], c["metric"], f32_bits(c["eps"]),
                                                                   c["table"], c["n"], c["film_mean"], c["film_m2"], c["score"]))
            else:
                f.write("target %s %d %d %d %d %d %d %d %d %d\n" % (name, c["width"], c["height"], f32_bits(c["target"]), c["c_min"], c["c_max"],
                                                                  c["error"], c["n"], c["sample_counts"], c["result"]))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("error") / "table.txt")
    write_table(path, table())
    return path, verdicts(build.ERROR_ARGS_BIN, path)


# ---------------------------------------------------------------- 1. the args header, alone
def test_the_table_states_every_error_and_valid_calls_of_both_entries():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid_"), (name, w)
    said = set(" ".join(w) for w in want.values() if w)
    assert len(said) >= 24, sorted(said)
    t = table()
    assert restated(t["error_metric_comes_before_table"]) == ["metric"] and restated(t["error_table_comes_before_eps"]) == ["table"]
    assert restated(t["error_eps_comes_before_null"]) == ["eps"]


def test_the_args_header_gives_the_restated_verdicts(args_out):
    _, out = args_out
    t = table()
    got = dict(line.split(" : ", 1) for line in out.splitlines())
    assert sorted(got) == sorted(t)
    for name, c in t.items():
        want = restated(c)
        if want is not None:
            assert not got[name].startswith("ok"), (name, got[name])
            for word in want:
                assert word in got[name], (name, word, got[name])
        elif c["kind"] == "error":
            vec = all(c[p] % 16 == 0 for p in ("n", "film_mean", "film_m2", "score"))
            assert got[name] == "ok error %d %d" % (vec, c["table"] >= 0), (name, got[name])
        else:
            chunks = -(-c["width"] * c["height"] // CHUNK)
            vec = int(all(c[p] % 16 == 0 for p in ("error", "n", "sample_counts")))
            assert got[name] == "ok target %d %d %d" % (chunks, min(chunks, MAX_GRID), vec), (name, got[name])
    # the message of an order case names the earlier argument only
    assert "table" not in got["error_metric_comes_before_table"] and "eps" not in got["error_table_comes_before_eps"]
    assert "target" not in got["target_alignment_comes_before_the_target"] and "c_min" not in got["target_the_target_comes_before_the_bounds"]


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "error_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


# ---------------------------------------------------------------- 2. the library, without a device
def test_symbols_are_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "int statmc_error_scores": "uint16_t width, uint16_t height, int channels, int metric, float eps, int table, const int32_t *n, "
                                   "const float *film_mean, const float *film_m2, float *score, void *stream",
        "int statmc_plan_to_target": "uint16_t width, uint16_t height, const float *error, const int32_t *n, float target, int32_t c_min, "
                                     "int32_t c_max, int32_t *sample_counts, statmc_target_result *result, void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl and " ".join(decl.group(1).split()) == args, sym
    body = re.search(r"typedef struct statmc_target_result \{(.*?)\} statmc_target_result;", header, re.S).group(1)
    fields = re.findall(r"(int64_t|uint32_t|int32_t)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [n.strip() for _, ns in fields for n in ns.split(",")]
    assert names == [f for f, _ in api.TargetResult._fields_] == ref.TARGET_RESULT_FIELDS
    tr = api.TargetResult
    assert C.sizeof(tr) == 48 and [getattr(tr, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 44]
    assert re.search(r"#define STATMC_ERROR_NO_TABLE \(-1\)", header) and api.ERROR_NO_TABLE == ref.NO_TABLE == -1
    assert "statmc_error.hip" in build.SOURCES and "statmc_error_args.h" in build.HEADERS
    assert callable(api.error_scores) and callable(api.plan_to_target) and callable(film.FilmStats.plan_to_target)
    import inspect
    for method in (film.FilmStats.plan_samples, film.FilmStats.score_quantiles, film.FilmStats.score_count_above):
        assert inspect.signature(method).parameters["error"].default is None, method
    # statmc_sample_scores stays what it was: the error of the mean is an entry of its own, not a third metric
    assert "statmc_error_scores" not in open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_plan.hip")).read()


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every invalid call of the table is refused with its argument named whether or not a
    device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        if c["kind"] == "error":
            call = lambda: lib.statmc_error_scores(c["width"], c["height"], c["channels"], c["metric"], c["eps"], c["table"], c["n"] or None,
                                                   c["film_mean"] or None, c["film_m2"] or None, c["score"] or None, None)
        else:
            call = lambda: lib.statmc_plan_to_target(c["width"], c["height"], c["error"] or None, c["n"] or None, c["target"], c["c_min"], c["c_max"],
                                                     c["sample_counts"] or None, C.cast(c["result"], C.POINTER(api.TargetResult)), None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_error_scores_gpu.py runs real ones)
            assert call() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- 3. the restatement's own properties
def test_error_restatement_matches_a_float64_evaluation_and_its_special_cases():
    rng = np.random.default_rng(2)
    n = rng.integers(0, 200, (16, 20)).astype(np.int32)
    mean = rng.normal(0, 1, (16, 20, 3)).astype(F32)
    m2 = (rng.random((16, 20, 3)) * 50).astype(F32)
    tq = ref.expand_table(1 + 64 / (np.arange(4096) + 1.0))
    for metric in (plan.ABSOLUTE, plan.RELATIVE):
        for t in (None, tq):
            e = ref.error_scores_ref(n, mean, m2, metric, 1e-3, t)
            assert e.dtype == F32 and np.all(np.isinf(e[n < 2])) and np.all(e[n < 2] > 0)
            ok = n >= 2
            want = np.sqrt(m2.astype(np.float64).sum(-1)[ok] / (n[ok] - 1) / n[ok])
            if t is not None:
                want = want * (1 + 64 / (n[ok] - 1.0))
            if metric == plan.RELATIVE:
                want = want / (1e-3 + np.abs(mean.astype(np.float64)).sum(-1)[ok])
            assert np.allclose(e[ok], want, rtol=2e-6, atol=0)
    m2[0, 0, 1] = np.nan
    m2[0, 1, :] = -1
    n[0, :2] = 5
    e = ref.error_scores_ref(n, mean, m2, plan.ABSOLUTE, 1e-3)
    assert np.isnan(e[0, 0]) and np.isnan(e[0, 1])
    # degrees of freedom: n - 1, the last entry from 4096 on; an 8-entry table repeats its last entry
    one = np.ones((1, 6, 1), F32)
    nn = np.array([[2, 3, 9, 10, 4097, 4098]], np.int32)
    base = ref.error_scores_ref(nn, one, one, plan.ABSOLUTE, 1e-3)
    full = ref.error_scores_ref(nn, one, one, plan.ABSOLUTE, 1e-3, tq) / base
    assert np.allclose(full, [65, 33, 9, 1 + 64 / 9, 1 + 64 / 4096, 1 + 64 / 4096], rtol=1e-6)
    short = ref.error_scores_ref(nn, one, one, plan.ABSOLUTE, 1e-3, ref.expand_table(tq[:8])) / base
    assert np.allclose(short, [65, 33, 9, 9, 9, 9], rtol=1e-6)


def test_at_n_equal_to_a_power_of_4_the_absolute_standard_error_is_the_score_scaled_bit_for_bit():
    """vm = v / 4^k is exact while v / 4^k is a normal number, and sqrt(v 4^-k) = sqrt(v) 2^-k exactly rounded alike."""
    rng = np.random.default_rng(3)
    mean = rng.normal(0, 1, (24, 40, 3)).astype(F32)
    m2 = np.exp(rng.normal(0, 4, (24, 40, 3))).astype(F32)
    for k in range(1, 12):
        n = np.full((24, 40), 4 ** k, np.int32)
        sd = plan.scores_ref(n, mean, m2, plan.ABSOLUTE, 1e-3)
        se = ref.error_scores_ref(n, mean, m2, plan.ABSOLUTE, 1e-3)
        assert np.array_equal(se.view(np.uint32), (sd * F32(2.0 ** -k)).view(np.uint32)), k


def plan_cases():
    rng = np.random.default_rng(7)
    h, w = 23, 31
    e = (plan.lognormal_scores(h, w, 4) * F32(0.05)).astype(F32)
    n = rng.integers(0, 200, (h, w)).astype(np.int32)
    mixed = e.copy()
    mixed.reshape(-1)[::7] = 0
    mixed.reshape(-1)[3::11] = np.inf
    mixed.reshape(-1)[5::13] = np.nan
    mixed.reshape(-1)[6::17] = -1
    return {"lognormal": (e, n), "mixed": (mixed, n)}


def test_counts_fall_as_the_target_rises_keep_their_bounds_and_sum_to_total():
    targets = [2.0 ** -60, 1e-6, 1e-3, 0.01, 0.02, 0.05, 0.2, 1.0, 1e6, 2.0 ** 60]
    for name, (e, n) in plan_cases().items():
        for c_min, c_max in ((0, 0), (0, 1 << 20), (1, 32)):
            before = None
            for t in targets:
                c, r = ref.plan_to_target_ref(e, n, t, c_min, c_max)
                assert c.dtype == np.int32 and c.min() >= c_min and c.max() <= c_max, (name, t)
                assert r["total"] == int(c.astype(np.int64).sum()), (name, t)
                live, sat = plan.classes(e)
                assert (r["n_live"], r["n_saturated"]) == (int(live.sum()), int(sat.sum()))
                assert 0 <= r["n_capped"] <= r["n_open"] <= r["n_live"] and r["n_unjudged"] >= r["n_saturated"]
                assert r["need"] >= 0 and (r["n_open"] > 0 or r["need"] == 0)
                if before is not None:
                    assert np.all(c <= before[0]) and r["need"] <= before[1]["need"] and r["n_open"] <= before[1]["n_open"], (name, t)
                before = (c, r)
        c, r = ref.plan_to_target_ref(e, n, 2.0 ** 60, 1, 32)
        assert r["n_open"] == 0 and r["need"] == 0      # no live error is above the largest target


def test_the_planned_total_brings_a_1_over_sqrt_n_error_to_the_target():
    """e(n) = s / sqrt(n): after N = n + d samples the error is at the target up to the roundings of r, r2, t."""
    rng = np.random.default_rng(9)
    s = np.exp(rng.normal(0, 1, (40, 50)))
    n = rng.integers(2, 500, (40, 50)).astype(np.int32)
    e = (s / np.sqrt(n)).astype(F32)
    t = 0.05
    c, r = ref.plan_to_target_ref(e, n, t, 0, 1 << 20)
    after = e.astype(np.float64) * np.sqrt(n / (n + c.astype(np.float64)))
    assert r["n_capped"] == 0 and r["n_open"] > 0
    assert np.all(after <= t * (1 + 1e-6))
    opened = e > F32(t)
    assert np.all(after[opened] >= t * np.sqrt(1 - 1.0 / (n + c)[opened]) * (1 - 1e-6))      # and not a sample more than needed


def quantile95(x):
    return float(np.sort(x.reshape(-1))[int(np.ceil(0.95 * x.size)) - 1])


def test_the_error_of_the_mean_falls_with_the_sample_count_and_the_sample_deviation_does_not():
    """iid synthetic statistics, 64 x 48, 8 and then 64 samples per pixel: the 95th percentile of the relative standard error falls
    by about sqrt(8) (measured 0.34 of its value); that of statmc_sample_scores' score stays where it is (0.97)."""
    q = {}
    for spp in (8, 64):
        n, mean, m2 = ref.iid_statistics(48, 64, spp, seed=11)
        q[spp] = (quantile95(ref.error_scores_ref(n, mean, m2, plan.RELATIVE, 1e-3)), quantile95(plan.scores_ref(n, mean, m2, plan.RELATIVE, 1e-3)))
    stderr_ratio, sd_ratio = q[64][0] / q[8][0], q[64][1] / q[8][1]
    print("95th percentile, 64 over 8 samples per pixel: standard error %.3f, sample deviation %.3f" % (stderr_ratio, sd_ratio))
    assert 0.25 <= stderr_ratio <= 0.45
    assert 0.8 <= sd_ratio <= 1.25
