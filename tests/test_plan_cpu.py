"""statmc_sample_scores / statmc_plan_samples (include/statmc.h) without a GPU: the symbols, their declarations and the ctypes
mirrors; the argument checks of statmc_amd/csrc/statmc_plan_args.h -- compiled alone into tests/cpp/test_plan_args.cpp, plain and under
AddressSanitizer and UBSan -- against a Python restatement of the header's rules; the workspace helper and what the built library
answers without a device; and the properties of the numpy float32 restatement (tests/plan_reference.py) that tests/test_plan_gpu.py
holds the device to."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import plan_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS_SRC = os.path.join(ROOT, "tests", "cpp", "test_plan_args.cpp")
F32 = np.float32
FW, FH = 64, 48
MIB = 1 << 20
N_AT, MEAN_AT, M2_AT, SCORE_AT, COUNTS_AT, RESULT_AT, WS_AT = (i * 16 * MIB for i in range(1, 8))   # made-up images, 16 MiB apart
PX = FW * FH * 4
CHUNK, WS_HEAD = 1024, 5 * 64 + 8      # pixels per scan block; 64-bit words in front of the block sums


def ws_bytes(w, h):
    return (WS_HEAD + -(-w * h // CHUNK)) * 8


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- the table of calls and the restatement of include/statmc.h
def scores(**kw):
    c = dict(kind="scores", width=FW, height=FH, channels=3, metric=1, eps=1e-3, n=N_AT, film_mean=MEAN_AT, film_m2=M2_AT, score=SCORE_AT)
    c.update(kw)
    return c


def plan(**kw):
    c = dict(kind="plan", width=FW, height=FH, budget=FW * FH * 8, c_min=1, c_max=32, score=SCORE_AT, n=N_AT, sample_counts=COUNTS_AT,
             result=RESULT_AT, workspace=WS_AT, workspace_bytes=None)
    c.update(kw)
    if c["workspace_bytes"] is None:
        c["workspace_bytes"] = ws_bytes(c["width"], c["height"]) if c["width"] and c["height"] else 0
    return c


def table():
    t = {}
    t["valid_scores"] = scores()
    t["valid_scores_one_channel_absolute"] = scores(channels=1, metric=0)
    t["valid_scores_absolute_ignores_eps"] = scores(metric=0, eps=-1.0)
    t["valid_scores_unaligned_plane"] = scores(film_m2=M2_AT + 4)
    t["valid_scores_odd_film"] = scores(width=37, height=29)
    t["valid_scores_score_right_behind_n"] = scores(score=N_AT + PX)
    t["scores_zero_width"] = scores(width=0)
    t["scores_zero_height"] = scores(height=0)
    t["scores_channels_2"] = scores(channels=2)
    t["scores_metric_2"] = scores(metric=2)
    t["scores_metric_minus_1"] = scores(metric=-1)
    for name, eps in (("zero", 0.0), ("negative", -1e-3), ("inf", float("inf")), ("nan", float("nan"))):
        t["scores_eps_" + name] = scores(eps=eps)
    for p in ("n", "film_mean", "film_m2", "score"):
        t["scores_null_" + p] = scores(**{p: 0})
        t["scores_misaligned_" + p] = scores(**{p: scores()[p] + 2})
    t["scores_score_is_n"] = scores(score=N_AT)
    t["scores_score_in_the_last_bytes_of_n"] = scores(score=N_AT + PX - 4)
    t["scores_score_in_the_last_bytes_of_film_mean"] = scores(score=MEAN_AT + 3 * PX - 4)
    t["valid_scores_score_right_behind_film_mean"] = scores(score=MEAN_AT + 3 * PX)
    t["scores_score_ends_inside_film_m2"] = scores(score=M2_AT - PX + 4)

    t["valid_plan"] = plan()
    t["valid_plan_without_n"] = plan(n=0)
    t["valid_plan_odd_film"] = plan(width=37, height=29)
    t["valid_plan_unaligned_counts"] = plan(sample_counts=COUNTS_AT + 4)
    t["valid_plan_zero_budget"] = plan(budget=0)
    t["valid_plan_zero_to_one"] = plan(c_min=0, c_max=1)
    t["valid_plan_equal_bounds"] = plan(c_min=7, c_max=7)
    t["valid_plan_largest_c_max"] = plan(c_max=1 << 20)
    t["valid_plan_larger_workspace"] = plan(workspace_bytes=ws_bytes(FW, FH) + 4096)
    far = dict(score=1 << 40, n=2 << 40, sample_counts=3 << 40, result=4 << 40, workspace=5 << 40)    # images of up to 16 GiB
    t["valid_plan_4k_film_narrow_sums"] = plan(width=3840, height=2160, c_max=(1 << 19) - 1, **far)      # 44 pixels per lane, 2816 per wave
    t["valid_plan_4k_film_wide_wave_sums"] = plan(width=3840, height=2160, c_max=1 << 20, **far)
    t["valid_plan_largest_film_narrow_lane_sums"] = plan(width=65535, height=65535, c_max=98000, **far)   # 21848 pixels per lane
    t["valid_plan_largest_film_wide_sums"] = plan(width=65535, height=65535, c_max=99000, **far)
    t["plan_zero_width"] = plan(width=0)
    t["plan_zero_height"] = plan(height=0)
    for p in ("score", "sample_counts", "result", "workspace"):
        t["plan_null_" + p] = plan(**{p: 0})
    for p in ("score", "n", "sample_counts"):
        t["plan_misaligned_" + p] = plan(**{p: plan()[p] + 2})
    t["plan_misaligned_result"] = plan(result=RESULT_AT + 4)
    t["plan_misaligned_workspace"] = plan(workspace=WS_AT + 4)
    t["plan_negative_c_min"] = plan(c_min=-1)
    t["plan_c_min_above_c_max"] = plan(c_min=9, c_max=8)
    t["plan_c_max_above_the_limit"] = plan(c_max=(1 << 20) + 1)
    t["plan_negative_budget"] = plan(budget=-1)
    t["plan_workspace_one_byte_short"] = plan(workspace_bytes=ws_bytes(FW, FH) - 1)
    t["plan_workspace_zero_bytes"] = plan(workspace_bytes=0)
    t["plan_counts_is_score"] = plan(sample_counts=SCORE_AT)
    t["plan_counts_is_n"] = plan(sample_counts=N_AT)
    t["plan_counts_in_the_last_bytes_of_score"] = plan(sample_counts=SCORE_AT + PX - 4)
    t["valid_plan_counts_right_behind_score"] = plan(sample_counts=SCORE_AT + PX)
    t["plan_counts_end_inside_n"] = plan(sample_counts=N_AT - PX + 4)
    t["valid_plan_counts_end_at_n"] = plan(sample_counts=N_AT - PX)
    t["plan_counts_over_result"] = plan(result=COUNTS_AT + 8)
    t["plan_counts_over_workspace"] = plan(workspace=COUNTS_AT + PX - 8)
    t["plan_result_inside_workspace"] = plan(result=WS_AT + 64)
    return t


def overlap(a, na, b, nb):
    return a != 0 and b != 0 and a < b + nb and b < a + na


def restated(c):
    """include/statmc.h's error lists: None for a valid call, else words the message must contain"""
    if c["width"] == 0 or c["height"] == 0:
        return ["width", "height"]
    px = c["width"] * c["height"] * 4
    if c["kind"] == "scores":
        if c["channels"] not in (1, 3):
            return ["channels"]
        if c["metric"] not in (0, 1):
            return ["metric"]
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
    for p in ("score", "sample_counts", "result", "workspace"):
        if c[p] == 0:
            return ["null " + p]
    for p, a in (("score", 4), ("n", 4), ("sample_counts", 4), ("result", 8), ("workspace", 8)):
        if c[p] % a:
            return [p, "aligned"]
    if not 0 <= c["c_min"] <= c["c_max"] <= 1 << 20:
        return ["c_min", "c_max"]
    if c["budget"] < 0:
        return ["budget"]
    need = ws_bytes(c["width"], c["height"])
    if c["workspace_bytes"] < need:
        return ["workspace_bytes", str(need)]
    for p, nb in (("score", px), ("n", px), ("result", 32), ("workspace", need)):
        if overlap(c["sample_counts"], px, c[p], nb):
            return ["sample_counts overlaps " + p]
    if overlap(c["result"], 32, c["workspace"], need):
        return ["result overlaps workspace"]
    return None


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def write_table(path, calls):
    with open(path, "w") as f:
        for name, c in calls.items():
            if c["kind"] == "scores":
                f.write("scores %s %d %d %d %d %d %d %d %d %d\n" % (name, c["width"], c["height"], c["channels"], c["metric"], f32_bits(c["eps"]),
                                                                 c["n"], c["film_mean"], c["film_m2"], c["score"]))
            else:
                f.write("plan %s %d %d %d %d %d %d %d %d %d %d %d\n" % (name, c["width"], c["height"], c["budget"], c["c_min"], c["c_max"], c["score"],
                                                                      c["n"], c["sample_counts"], c["result"], c["workspace"], c["workspace_bytes"]))


def verdicts(binary, path):
    out = subprocess.run([binary, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def args_out(tmp_path_factory):
    from statmc_amd import build
    build.build_tools()
    path = str(tmp_path_factory.mktemp("plan") / "table.txt")
    write_table(path, table())
    return path, verdicts(build.PLAN_ARGS_BIN, path)


# ---------------------------------------------------------------- 1. the args header, alone
def test_the_table_states_every_error_and_valid_calls_of_both_entries():
    want = {name: restated(c) for name, c in table().items()}
    for name, w in want.items():
        assert (w is None) == name.startswith("valid_"), (name, w)
    said = set(" ".join(w) for w in want.values() if w)
    assert len(said) >= 25, sorted(said)


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
        elif c["kind"] == "scores":
            vec = all(c[p] % 16 == 0 for p in ("n", "film_mean", "film_m2", "score"))
            assert got[name] == "ok scores %d" % vec, (name, got[name])
        else:
            chunks = -(-c["width"] * c["height"] // CHUNK)
            grid = min(chunks, 768)
            px_per_lane = -(-chunks // grid) * 4
            wide = int(px_per_lane * c["c_max"] >= 1 << 31)      # a lane's int32 partial sums could leave 31 bits
            wide_wave = int(64 * px_per_lane * c["c_max"] >= 1 << 31)      # ... the sums of a wave's 64 lanes
            vec = int(all(c[p] % 16 == 0 for p in ("score", "n", "sample_counts")))
            assert got[name] == "ok plan %d %d %d %d %d %d" % (ws_bytes(c["width"], c["height"]), chunks, grid, wide, wide_wave, vec), (name, got[name])
    sums = lambda name: got[name].split()[5:7]
    assert sums("valid_plan") == ["0", "0"] and sums("valid_plan_4k_film_narrow_sums") == ["0", "0"]
    assert sums("valid_plan_4k_film_wide_wave_sums") == ["0", "1"] and sums("valid_plan_largest_film_narrow_lane_sums") == ["0", "1"]
    assert sums("valid_plan_largest_film_wide_sums") == ["1", "1"]


def test_the_args_program_is_clean_under_sanitizers(args_out, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own: no
    report, the same lines."""
    path, plain = args_out
    binary = str(tmp_path / "plan_args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "include"), ARGS_SRC, "-o", binary])
    assert verdicts(binary, path) == plain


# ---------------------------------------------------------------- 2. the library, without a device
def test_symbols_are_exported_declared_and_mirrored(lib):
    from statmc_amd import api, build, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decls = {
        "int statmc_sample_scores": "uint16_t width, uint16_t height, int channels, int metric, float eps, const int32_t *n, "
                                    "const float *film_mean, const float *film_m2, float *score, void *stream",
        "size_t statmc_plan_samples_workspace": "uint16_t width, uint16_t height",
        "int statmc_plan_samples": "uint16_t width, uint16_t height, const float *score, const int32_t *n, int64_t budget, int32_t c_min, "
                                   "int32_t c_max, int32_t *sample_counts, statmc_plan_result *result, void *workspace, size_t workspace_bytes, "
                                   "void *stream",
    }
    for head, args in decls.items():
        sym = head.split()[-1]
        assert hasattr(lib, sym) and sym in api.EXPORTS, sym
        decl = re.search(re.escape(head) + r"\s*\(([^;]*)\)\s*;", header)
        assert decl and " ".join(decl.group(1).split()) == args, sym
    body = re.search(r"typedef struct statmc_plan_result \{(.*?)\} statmc_plan_result;", header, re.S).group(1)
    fields = re.findall(r"(int64_t|uint32_t|int32_t)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [n.strip() for _, ns in fields for n in ns.split(",")]
    assert names == [f for f, _ in api.PlanResult._fields_] == ["total", "budget", "level_bits", "status", "n_live", "n_saturated"]
    pr = api.PlanResult
    assert C.sizeof(pr) == 32 and [getattr(pr, f).offset for f in names] == [0, 8, 16, 20, 24, 28]
    assert re.search(r"#define STATMC_SCORE_ABSOLUTE 0\b", header) and re.search(r"#define STATMC_SCORE_RELATIVE 1\b", header)
    assert (api.SCORE_ABSOLUTE, api.SCORE_RELATIVE) == (ref.ABSOLUTE, ref.RELATIVE) == (0, 1)
    assert (api.PLAN_LEVEL_LO, api.PLAN_LEVEL_HI, api.PLAN_MAX_COUNT) == (ref.U_LO, ref.U_HI, ref.MAX_COUNT)
    assert "statmc_plan.hip" in build.SOURCES and "statmc_plan_args.h" in build.HEADERS
    assert callable(api.sample_scores) and callable(api.plan_samples) and callable(film.FilmStats.plan_samples)


def test_the_workspace_helper_needs_no_device(lib):
    from statmc_amd import api
    for w, h in ((1, 1), (37, 29), (64, 48), (257, 131), (1920, 1080), (3840, 2160), (65535, 65535)):
        assert api.plan_samples_workspace(w, h) == ws_bytes(w, h), (w, h)
    assert api.plan_samples_workspace(1920, 1080) < 32 * 1024     # the search's totals and one word per 1024 pixels


def test_without_a_device_the_entries_check_their_arguments_first(lib):
    """Made-up pointers, never dereferenced.  Every invalid call of the table is refused with its argument named whether or not a
    device is set up; a valid call gets as far as the device check."""
    import torch
    from statmc_amd import api
    for name, c in table().items():
        want = restated(c)
        if c["kind"] == "scores":
            call = lambda: lib.statmc_sample_scores(c["width"], c["height"], c["channels"], c["metric"], c["eps"], c["n"] or None,
                                                    c["film_mean"] or None, c["film_m2"] or None, c["score"] or None, None)
        else:
            call = lambda: lib.statmc_plan_samples(c["width"], c["height"], c["score"] or None, c["n"] or None, c["budget"], c["c_min"], c["c_max"],
                                                   c["sample_counts"] or None, C.cast(c["result"], C.POINTER(api.PlanResult)),
                                                   c["workspace"] or None, c["workspace_bytes"], None)
        if want is not None:
            assert call() == api.ERR_INVALID, name
            msg = lib.statmc_last_error().decode()
            for word in want:
                assert word in msg, (name, word, msg)
        elif not torch.cuda.is_available():     # a valid call would run on made-up pointers (tests/test_plan_gpu.py runs real ones)
            assert call() == api.ERR_NO_DEVICE, name
            assert b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- 3. the restatement's own properties
def film_cases():
    rng = np.random.default_rng(5)
    h, w = 23, 31
    logn = ref.lognormal_scores(h, w, 1)
    n = rng.integers(0, 40, (h, w)).astype(np.int32)
    mixed = logn.copy()
    mixed.reshape(-1)[::7] = 0
    mixed.reshape(-1)[3::11] = np.inf
    mixed.reshape(-1)[5::13] = np.nan
    mixed.reshape(-1)[6::17] = -1
    return {"lognormal": (logn, n, 1, 64), "lognormal_no_n": (logn, None, 0, 50), "mixed": (mixed, n, 2, 33),
            "constant": (np.full((h, w), 0.75, F32), None, 0, 1000)}


def test_scores_restatement_matches_a_float64_evaluation_and_its_special_cases():
    rng = np.random.default_rng(2)
    n = rng.integers(0, 200, (16, 20)).astype(np.int32)
    mean = rng.normal(0, 1, (16, 20, 3)).astype(F32)
    m2 = (rng.random((16, 20, 3)) * 50).astype(F32)
    for metric in (ref.ABSOLUTE, ref.RELATIVE):
        s = ref.scores_ref(n, mean, m2, metric, 1e-3)
        assert s.dtype == F32 and np.all(np.isinf(s[n < 2])) and np.all(s[n < 2] > 0)
        ok = n >= 2
        want = np.sqrt(m2.astype(np.float64).sum(-1)[ok] / (n[ok] - 1))
        if metric == ref.RELATIVE:
            want = want / (1e-3 + np.abs(mean.astype(np.float64)).sum(-1)[ok])
        assert np.allclose(s[ok], want, rtol=1e-6, atol=0)
    m2[0, 0, 1] = np.nan
    m2[0, 1, :] = -1
    n[0, :2] = 5
    s = ref.scores_ref(n, mean, m2, ref.ABSOLUTE, 1e-3)
    assert np.isnan(s[0, 0]) and np.isnan(s[0, 1])


def test_T_is_monotone_in_the_level():
    for name, (s, n, c_min, c_max) in film_cases().items():
        us = np.unique(np.concatenate([np.linspace(ref.U_LO, ref.U_HI, 400).astype(np.int64),
                                       np.arange(0x3F800000 - 40, 0x3F800000 + 40), [ref.U_LO, ref.U_LO + 1, ref.U_HI - 1, ref.U_HI]]))
        T = [ref.total_at(int(u), s, n, c_min, c_max) for u in us]
        assert all(a <= b for a, b in zip(T, T[1:])), name
        live, sat = ref.classes(s)
        dead = s.size - int(live.sum()) - int(sat.sum())
        assert T[0] >= s.size * c_min and T[-1] <= s.size * c_max and T[-1] >= int(sat.sum()) * c_max + dead * c_min, name


def test_status_0_spends_the_budget_to_the_sample_and_every_count_keeps_its_bounds():
    for name, (s, n, c_min, c_max) in film_cases().items():
        lo, hi = ref.total_at(ref.U_LO, s, n, c_min, c_max), ref.total_at(ref.U_HI, s, n, c_min, c_max)
        assert lo < hi, name
        for budget in sorted({lo + 1, hi, (lo + hi) // 2, lo + (hi - lo) // 3, lo + 17}):
            c, r = ref.plan_ref(s, n, budget, c_min, c_max)
            assert r["status"] == 0 and r["total"] == budget == int(c.astype(np.int64).sum()), (name, budget)
            assert c.dtype == np.int32 and c.min() >= c_min and c.max() <= c_max, (name, budget)
            assert ref.total_at(r["level_bits"], s, n, c_min, c_max) >= budget > ref.total_at(r["level_bits"] - 1, s, n, c_min, c_max)
        for budget, status, level in ((0, 1, ref.U_LO), (lo, 1, ref.U_LO), (hi + 1, 2, ref.U_HI), (10 ** 12, 2, ref.U_HI)):
            c, r = ref.plan_ref(s, n, budget, c_min, c_max)
            assert (r["status"], r["level_bits"], r["budget"]) == (status, level, budget), (name, budget)
            assert r["total"] == (lo if status == 1 else hi) == int(c.astype(np.int64).sum())
            assert np.array_equal(c, ref.counts_at(level, s, n, c_min, c_max))


def test_a_budget_equal_to_some_T_takes_that_level_whole():
    s, n, c_min, c_max = film_cases()["lognormal"]
    u = 0x40A00000     # level 5.0
    budget = ref.total_at(u, s, n, c_min, c_max)
    c, r = ref.plan_ref(s, n, budget, c_min, c_max)
    assert r["status"] == 0 and r["level_bits"] <= u and np.array_equal(c, ref.counts_at(r["level_bits"], s, n, c_min, c_max))


def test_on_a_constant_film_the_trim_hands_the_last_samples_to_the_first_pixels_in_raster_order():
    s, n, c_min, c_max = film_cases()["constant"]
    px = s.size
    for budget in (px * 10 + 1, px * 10 + 100, px * 11 - 1, px * 11):
        c, r = ref.plan_ref(s, n, budget, c_min, c_max)
        q, extra = divmod(budget, px)
        flat = c.reshape(-1)
        if extra == 0:
            assert np.all(flat == q)
        else:
            assert np.all(flat[:extra] == q + 1) and np.all(flat[extra:] == q), budget
        assert r["status"] == 0 and r["n_live"] == px and r["n_saturated"] == 0


def test_the_level_is_optimal_up_to_one_float_step():
    """What the ceil rule guarantees, and why.  With L = float(u*), L' = float(u* - 1) and N_p = n_p + c_p: a live pixel p that could
    take a sample (c_p < c_max) has N_p >= fl(L' s_p), a live pixel q that could give one (c_q > c_min) has N_q - 1 < fl(L s_q).  So
    s_p / N_p <= (1 / L') (1 + 2^-24) and s_q / (N_q - 1) > (1 / L) (1 - 2^-24): p as it stands is at least as well sampled per unit
    of score as q would be after giving a sample away, up to L / L' <= 1 + 2^-23 and the products' roundings.  In variances:
    the gain of the move, s_p^2 / (N_p (N_p + 1)) < (s_p / N_p)^2, stays below (s_q / (N_q - 1))^2 (1 + 2^-21), which is the move's
    cost s_q^2 / (N_q (N_q - 1)) times N_q / (N_q - 1): no transfer gains more than the last-sample granularity of the giver."""
    slack = 1 + 2.0 ** -21
    for name, (s, n, c_min, c_max) in film_cases().items():
        if name == "constant":
            continue
        lo, hi = ref.total_at(ref.U_LO, s, n, c_min, c_max), ref.total_at(ref.U_HI, s, n, c_min, c_max)
        for budget in (lo + (hi - lo) // 5, (lo + hi) // 2):
            c, r = ref.plan_ref(s, n, budget, c_min, c_max)
            live, _ = ref.classes(s)
            N = c.astype(np.float64) + (0 if n is None else np.clip(n, 0, None))
            s64 = s.astype(np.float64)
            take = live & (c < c_max)
            give = live & (c > c_min)
            assert take.any() and give.any(), name
            worst_taker = (s64[take] / N[take]).max()                 # (a taker has N >= 1: fl(L' s) > 0)
            with np.errstate(divide="ignore"):
                best_giver = (s64[give] / (N[give] - 1)).min()        # (a giver with N = 1 would leave nothing: inf)
            assert worst_taker <= best_giver * slack, (name, budget, worst_taker, best_giver)
            gain = (s64[take] ** 2 / (N[take] * (N[take] + 1))).max()
            assert gain <= best_giver ** 2 * slack, (name, budget)
