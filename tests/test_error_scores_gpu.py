"""statmc_error_scores / statmc_plan_to_target on the device against the numpy float32 restatement of include/statmc.h
(tests/error_reference.py, whose own properties tests/test_error_scores_cpu.py checks): error scores and counts bit for bit, every
field of the result, determinism, a library stream, the identity against statmc_sample_scores, and the upper layers: FilmStats, the C++
Estimator's scoreOf / PlanToTarget and the render loop's --stop-metric / --target-error.

One allowance, tests/test_plan_gpu.py's, for NaN only: where the restatement's score is NaN the device's must be NaN, whichever sign
and payload.  Every other score is held to the bit."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import error_reference as ref
import plan_reference as plan
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
SCORE_FILMS = [(37, 29), (64, 48)]             # element tails and a partial last quad; aligned
PLAN_FILMS = [(37, 29), (64, 48), (257, 131)]  # ... and several workgroups
FIELDS = ref.TARGET_RESULT_FIELDS


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()     # (the shared inputs and plans are read-only)


def dev_offset(a):
    """the same values in an image that starts 4 bytes into its allocation: 4-byte but not 16-byte aligned"""
    import torch
    flat = dev(np.asarray(a).reshape(-1))
    buf = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda:0")
    view = buf[1:1 + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(a.shape)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


def same_scores(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---------------------------------------------------------------- error scores
def statistics(W, H, ch, seed):
    """tests/test_plan_gpu.py's statistics() draw, plus the edges of this kernel's n: the degrees of freedom around the table's ends
    and counts that (float) rounds"""
    rng = np.random.default_rng(seed)
    special = np.array([0, 1, 2, 3, 4, 7, 100, 65536, (1 << 24) - 1, 1 << 24,
                        -5, 9, 10, 4096, 4097, 4098, (1 << 24) + 1], np.int32)
    n = rng.integers(0, 300, (H, W)).astype(np.int32)
    pick = rng.random((H, W)) < 0.5
    n[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    n.reshape(-1)[:len(special)] = special          # every edge at least once, whatever the draw
    mean = rng.normal(0, 2, (H, W, ch)).astype(F32)
    mean[rng.random(mean.shape) < 0.1] = 0
    m2 = (rng.lognormal(0, 2, (H, W, ch)) * np.maximum(n, 1)[..., None]).astype(F32)
    u = rng.random(m2.shape)
    m2[u < 0.10] = 0
    m2[(u >= 0.10) & (u < 0.13)] = -m2[(u >= 0.10) & (u < 0.13)]
    m2[(u >= 0.13) & (u < 0.15)] = np.nan
    m2[(u >= 0.15) & (u < 0.17)] = np.inf
    m2[(u >= 0.17) & (u < 0.19)] = F32(1e-42)       # subnormal sums, quotients and products
    m2[(u >= 0.19) & (u < 0.21)] = F32(3e-38)       # a normal m2 whose v / n is subnormal
    mean[(u >= 0.21) & (u < 0.22)] = np.inf
    n[1, :4], m2[1, :4], mean[1, :4] = 50, 0, 1      # a zero score, whatever the draw
    return n, mean, m2


def load_table(gpu, table, quantiles):
    q = np.ascontiguousarray(quantiles, F32)
    gpu.check(gpu.load().statmc_set_t_quantiles(table, q.ctypes.data_as(C.POINTER(C.c_float)), q.size))


def restore_tables(gpu):
    for t in range(6):
        gpu.check(gpu.load().statmc_set_t_quantiles(t, None, 0))


FULL_TABLE = (1 + 64 / (np.arange(4096) + 1.0)).astype(F32)      # distinct values: an off-by-one in the index shows


@pytest.mark.parametrize("table", [-1, 0, 5])
@pytest.mark.parametrize("metric", ["absolute", "relative"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("film", SCORE_FILMS, ids=lambda f: "%dx%d" % f)
def test_error_scores_equal_the_restatement_bit_for_bit(gpu, film, ch, metric, table):
    import torch
    W, H = film
    n, mean, m2 = statistics(W, H, ch, seed=W + ch)
    eps = 1e-3
    d_n, d_mean, d_m2 = dev(n), dev(mean if ch == 3 else mean[..., 0]), dev(m2 if ch == 3 else m2[..., 0])
    loads = [None] if table < 0 else [FULL_TABLE, FULL_TABLE[:8]]      # n_dof = 8: larger degrees of freedom reuse the last entry
    assert len(np.unique(FULL_TABLE)) == 4096
    try:
        for quantiles in loads:
            on_device = None
            if quantiles is not None:
                load_table(gpu, table, quantiles)
                on_device = ref.expand_table(quantiles)
            want = ref.error_scores_ref(n, mean, m2, gpu._METRICS[metric], eps, on_device)
            assert np.isinf(want).any() and np.isnan(want).any() and (want == 0).any() and (np.isfinite(want) & (want > 0)).sum() > W * H // 4
            assert ((m2 > 0) & (m2 < F32(1.1e-38)) & (n >= 2)[..., None]).any()      # subnormal m2, quotients and products are part of the definition
            got = gpu.error_scores(d_n, d_mean, d_m2, metric=metric, eps=eps, table=table)
            torch.cuda.synchronize()
            same_scores(got.cpu().numpy(), want)
            # the element path: one plane 4 bytes off the 16-byte grid, same bits
            out = dev_offset(np.zeros((H, W), F32))
            if ch == 3:
                gpu.error_scores(d_n, d_mean, dev_offset(m2), metric=metric, eps=eps, table=table, out=out)
            else:
                gpu.error_scores(dev_offset(n), d_mean, d_m2, metric=metric, eps=eps, table=table, out=out)
            torch.cuda.synchronize()
            same_scores(out.cpu().numpy(), want)
    finally:
        restore_tables(gpu)


def test_the_built_in_two_sided_table_widens_the_standard_error(gpu):
    """no table loaded: the half-width is the standard error times a quantile above 1, larger at few degrees of freedom"""
    import torch
    restore_tables(gpu)
    n = np.array([[2, 3, 10, 100, 5000, 1 << 20, 30, 30]], np.int32)
    one = np.ones((1, 8, 1), F32)
    se = gpu.error_scores(dev(n), dev(one), dev(one), metric="absolute", table=-1).cpu().numpy()
    ci = gpu.error_scores(dev(n), dev(one), dev(one), metric="absolute", table=gpu.get_significance()).cpu().numpy()
    assert np.array_equal(ci, gpu.error_scores(dev(n), dev(one), dev(one), metric="absolute", table="ci").cpu().numpy())
    torch.cuda.synchronize()
    q = (ci / se).reshape(-1)       # the quantile up to the quotient's rounding
    assert np.all(q > 1) and np.all(np.diff(q[:5]) < 0) and abs(q[4] / q[5] - 1) < 1e-6 and q[6] == q[7]


def test_at_n_equal_to_a_power_of_4_the_absolute_standard_error_is_sample_scores_scaled_bit_for_bit(gpu):
    import torch
    rng = np.random.default_rng(3)
    H, W = 24, 40
    mean = rng.normal(0, 1, (H, W, 3)).astype(F32)
    m2 = np.exp(rng.normal(0, 4, (H, W, 3))).astype(F32)
    k = np.broadcast_to(np.arange(1, 13).repeat(2)[:, None], (H, W))
    n = (4 ** k).astype(np.int32)
    d = (dev(n), dev(mean), dev(m2))
    sd = gpu.sample_scores(*d, metric="absolute")
    se = gpu.error_scores(*d, metric="absolute", table=-1)
    torch.cuda.synchronize()
    want = sd.cpu().numpy() * (F32(2.0) ** (-k).astype(F32))
    assert np.all(np.isfinite(want)) and np.all(want > F32(1.2e-38))
    assert np.array_equal(bits(se), bits(want))


# ---------------------------------------------------------------- plans to a target
def next_up(x, k=1):
    return (np.array([x], F32).view(np.int32) + k).view(F32)[0]


TARGETS = [2.0 ** -60, 0.01, 1.0, 2.0 ** 60]
BOUNDS = [(0, 0), (0, 1 << 20), (1, 32)]
_inputs, _plans = {}, {}


def plan_inputs(W, H):
    """(error, n): lognormal errors around every target of TARGETS with the specials of the classes, the targets themselves and the
    next float above each; n with its own edges.  Made once per film and left unchanged."""
    if (W, H) not in _inputs:
        rng = np.random.default_rng(W * 1000 + H)
        px = W * H
        e = plan.lognormal_scores(H, W, seed=W).reshape(-1)
        scale = np.array([0.01, 1.0, 2.0 ** -58, 2.0 ** 57], F32)[rng.integers(0, 4, px)]
        e = (e * scale).astype(F32)
        special = [0, -1, np.nan, np.inf, -np.inf, 2.0 ** -61, 2.0 ** -60, 2.0 ** 60, 2.0 ** 61]
        for t in TARGETS:
            special += [F32(t), next_up(F32(t)), next_up(F32(t), -1)]
        special = np.array(special, F32)
        pick = rng.random(px) < 0.3
        e[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        n_special = np.array([-3, 0, 1, 2, (1 << 24) + 1, 1 << 30, np.iinfo(np.int32).max], np.int32)
        n = rng.integers(2, 400, px).astype(np.int32)
        pick = rng.random(px) < 0.3
        n[pick] = n_special[rng.integers(0, len(n_special), int(pick.sum()))]
        # every special error against every special n, whatever the draw
        k = len(special) * len(n_special)
        assert k <= px
        e[:k] = np.repeat(special, len(n_special))
        n[:k] = np.tile(n_special, len(special))
        e, n = e.reshape(H, W), n.reshape(H, W)
        e.setflags(write=False)
        n.setflags(write=False)
        _inputs[(W, H)] = (e, n)
    return _inputs[(W, H)]


def planned(film, target, bounds):
    """the restatement's (counts, result), computed once and left unchanged"""
    key = (film, target, bounds)
    if key not in _plans:
        e, n = plan_inputs(*film)
        want = ref.plan_to_target_ref(e, n, target, *bounds)
        want[0].setflags(write=False)
        _plans[key] = want
    return _plans[key]


@pytest.mark.parametrize("bounds", BOUNDS, ids=lambda b: "%d_to_%d" % b)
@pytest.mark.parametrize("target", TARGETS, ids=["2^-60", "0.01", "1", "2^60"])
@pytest.mark.parametrize("film", PLAN_FILMS, ids=lambda f: "%dx%d" % f)
def test_plan_to_target_equals_the_restatement_bit_for_bit(gpu, film, target, bounds):
    e, n = plan_inputs(*film)
    want, want_res = planned(film, target, bounds)
    got, res = gpu.plan_to_target(dev(e), dev(n), target, bounds[0], bounds[1], return_result=True)
    got = got.cpu().numpy()
    assert {k: res[k] for k in FIELDS} == want_res
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got.min() >= bounds[0] and got.max() <= bounds[1] and res["total"] == int(got.astype(np.int64).sum())
    assert res["n_live"] > 0 and res["n_saturated"] > 0 and res["n_unjudged"] > res["n_saturated"]
    if target < 2.0 ** 60:
        assert 0 < res["n_open"] < res["n_live"] and res["need"] > 0
    if bounds == (1, 32) and target <= 1.0:
        assert 0 < res["n_capped"] <= res["n_open"]


def test_counts_fall_as_the_target_rises_on_the_device(gpu):
    film = PLAN_FILMS[2]
    e, n = plan_inputs(*film)
    d_e, d_n = dev(e), dev(n)
    before = None
    for t in TARGETS:
        c = gpu.plan_to_target(d_e, d_n, t, 0, 1 << 20).cpu().numpy()
        assert before is None or np.all(c <= before)
        before = c


@pytest.mark.parametrize("film", PLAN_FILMS, ids=lambda f: "%dx%d" % f)
def test_same_bits_on_every_run_with_a_garbage_result_unaligned_and_on_a_library_stream(gpu, film):
    import torch
    lib = gpu.load()
    e, n = plan_inputs(*film)
    target, bounds = 0.01, (1, 32)
    want, want_res = planned(film, target, bounds)
    d_e, d_n = dev(e), dev(n)
    first, res1 = gpu.plan_to_target(d_e, d_n, target, *bounds, return_result=True)
    second, res2 = gpu.plan_to_target(d_e, d_n, target, *bounds, return_result=True)
    assert np.array_equal(first.cpu().numpy(), want) and np.array_equal(second.cpu().numpy(), want) and res1 == res2
    assert {k: res1[k] for k in FIELDS} == want_res
    # a result full of garbage before the call
    garbage = torch.full((6,), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda:0")
    third, res3 = gpu.plan_to_target(d_e, d_n, target, *bounds, result=garbage, return_result=True)
    assert np.array_equal(third.cpu().numpy(), want) and res3 == res1
    # the element path: every image 4 bytes off the 16-byte grid
    out = dev_offset(np.full(e.shape, -1, np.int32))
    _, res4 = gpu.plan_to_target(dev_offset(e), dev_offset(n), target, *bounds, out=out, return_result=True)
    assert np.array_equal(out.cpu().numpy(), want) and res4 == res1
    # a library stream
    out = torch.full(e.shape, -1, dtype=torch.int32, device="cuda:0")
    result = torch.full((6,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stream = C.c_void_p()
    gpu.check(lib.statmc_stream_create(C.byref(stream)))
    try:
        _, res5 = gpu.plan_to_target(d_e, d_n, target, *bounds, out=out, result=result, stream=stream, return_result=True)
    finally:
        gpu.check(lib.statmc_stream_destroy(stream))
    assert np.array_equal(out.cpu().numpy(), want) and res5 == res1


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    e = torch.ones(8, 8, device="cuda:0")
    n = torch.ones(8, 8, dtype=torch.int32, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="c_min"):
        gpu.plan_to_target(e, n, 0.1, 5, 4)
    with pytest.raises(gpu.StatmcError, match="target"):
        gpu.plan_to_target(e, n, 0.0, 0, 4)
    with pytest.raises(gpu.StatmcError, match="target"):
        gpu.plan_to_target(e, n, float("nan"), 0, 4)
    with pytest.raises(gpu.StatmcError, match="table"):
        gpu.error_scores(n, e, e.clone(), table=6)
    with pytest.raises(gpu.StatmcError, match="eps"):
        gpu.error_scores(n, e, e.clone(), eps=0.0)
    with pytest.raises(gpu.StatmcError, match="metric"):     # statmc_sample_scores stays as it was: no third metric
        gpu.sample_scores(n, e, e.clone(), metric=2)


# ---------------------------------------------------------------- FilmStats
def test_film_stats_plans_to_a_target_what_its_counted_accumulation_takes(gpu):
    import torch
    from statmc_amd.film import FilmStats
    W, H, CAP = 64, 48, 16
    names = ("radiance", "normal", "albedo")
    scene, smp, _ = make_case(W, H, 8)
    arena = {k: v.numpy() for k, v in scene.samples(CAP, seed=991, features=names).items()}
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names})
    rad = film.state["radiance"]
    host = [rad[k].cpu().numpy() for k in ("n", "film_mean", "film_m2")]

    # error=None: the three methods return what they return without the argument
    q = [0.5, 0.95]
    sd = film.score_quantiles(q)
    assert np.array_equal(sd, film.score_quantiles(q, error=None))
    score = gpu.sample_scores(rad["n"], rad["film_mean"], rad["film_m2"])
    px = W * H
    ranks = [int(np.ceil(x * px)) - 1 for x in q]
    assert np.array_equal(bits(sd), bits(gpu.read_select_result(gpu.score_select(score, ranks))["values"]))
    assert film.score_count_above([float(sd[0])]) == film.score_count_above([float(sd[0])], error=None) == \
        [int(c) for c in gpu.score_count_above(score, [float(sd[0])]).cpu().numpy()]
    c0, r0 = film.plan_samples(px * 8, 1, CAP, return_result=True)
    c1, r1 = film.plan_samples(px * 8, 1, CAP, return_result=True, error=None)
    want, _ = plan.plan_ref(plan.scores_ref(*host, plan.RELATIVE, 1e-3), host[0], px * 8, 1, CAP)
    assert np.array_equal(c0.cpu().numpy(), want) and np.array_equal(c1.cpu().numpy(), want) and r0 == r1

    # error="stderr": score_select on error_scores
    errors = gpu.error_scores(rad["n"], rad["film_mean"], rad["film_m2"], table=-1)
    same_scores(errors.cpu().numpy(), ref.error_scores_ref(*host, plan.RELATIVE, 1e-3))
    se = film.score_quantiles(q, error="stderr")
    assert np.array_equal(bits(se), bits(gpu.read_select_result(gpu.score_select(errors, ranks))["values"]))
    assert np.all(se < sd) and np.all(film.score_quantiles(q, error="ci") > se)
    assert film.score_count_above([float(se[0])], error="stderr") == [int(c) for c in gpu.score_count_above(errors, [float(se[0])]).cpu().numpy()]
    with pytest.raises(ValueError):
        film.score_quantiles(q, error="variance")

    # plan_to_target: the restatement's counts, and they go into accumulate(samples, counts=)
    target = float(se[0])       # the median standard error: half the film is open
    counts, res = film.plan_to_target(target, 1, CAP, error="stderr", return_result=True)
    want, want_res = ref.plan_to_target_ref(errors.cpu().numpy(), host[0], target, 1, CAP)
    assert np.array_equal(counts.cpu().numpy(), want) and {k: res[k] for k in FIELDS} == want_res and not res["by_budget"]
    assert 0 < res["n_open"] < px and len(np.unique(want)) > 3
    assert np.array_equal(film.plan_to_target(target, 1, CAP, error="stderr").cpu().numpy(), want)
    n_before = host[0].copy()
    film.accumulate({t: dev(arena[t]) for t in names}, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(film.state["radiance"]["n"].cpu().numpy() - n_before, want)
    # the budget: one that fits keeps the plan, one that does not is spent as plan_samples spends it
    film2 = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film2.accumulate({t: dev(smp[t]) for t in names})
    fits, res_fits = film2.plan_to_target(target, 1, CAP, budget=want_res["total"], error="stderr", return_result=True)
    assert np.array_equal(fits.cpu().numpy(), want) and not res_fits["by_budget"]
    short, res_short = film2.plan_to_target(target, 1, CAP, budget=want_res["total"] - 1, error="stderr", return_result=True)
    by_budget, _ = plan.plan_ref(plan.scores_ref(*host, plan.RELATIVE, 1e-3), host[0], want_res["total"] - 1, 1, CAP)
    assert res_short["by_budget"] and np.array_equal(short.cpu().numpy(), by_budget) and res_short["budgeted"]["total"] == want_res["total"] - 1
    assert {k: res_short[k] for k in FIELDS} == want_res


# ---------------------------------------------------------------- the C++ Estimator
def test_estimator_plans_to_a_target_what_the_python_entry_plans(gpu, tmp_path):
    """C++ host (tests/cpp/test_plan_to_target.cpp): reuse and staleness of the score image across scoreOf and after
    statmc_set_significance, the budget fallback; PlanToTarget's counts and result equal the Python entries' for the statistics it
    dumps."""
    from statmc_amd import build
    build.build_tools()
    W, H, TARGET = 61, 37, 0.03
    prefix = str(tmp_path / "target")
    out = subprocess.run([build.TARGET_BIN, str(W), str(H), repr(TARGET), prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan to target ok" in out.stdout
    n = np.fromfile(prefix + ".n.i32", np.int32).reshape(H, W)
    mean = np.fromfile(prefix + ".film_mean.f32", F32).reshape(H, W, 3)
    m2 = np.fromfile(prefix + ".film_m2.f32", F32).reshape(H, W, 3)
    counts = np.fromfile(prefix + ".counts.i32", np.int32).reshape(H, W)
    m = re.search(r"target: total (\d+) need (\d+) n_open (\d+) n_capped (\d+) n_unjudged (\d+) n_live (\d+) n_saturated (\d+)", out.stdout)
    errors = gpu.error_scores(dev(n), dev(mean), dev(m2), metric="relative", eps=1e-3, table="stderr")
    got, res = gpu.plan_to_target(errors, dev(n), TARGET, 1, 64, return_result=True)
    assert np.array_equal(got.cpu().numpy(), counts) and len(np.unique(counts)) > 2
    assert [res[k] for k in FIELDS] == [int(g) for g in m.groups()]
    want, want_res = ref.plan_to_target_ref(ref.error_scores_ref(n, mean, m2, plan.RELATIVE, 1e-3), n, TARGET, 1, 64)
    assert np.array_equal(counts, want) and res == want_res


# ---------------------------------------------------------------- the render loop
SIM_LINES = ("Target:", "Spent:", "Iteration:", "SPP:", "Rendering time [ns]:", "CUDA time [ns]:", "Planned:", "Output time [ns]:", "Staged bytes:",
             "Converged:")


def run_sim(build, *flags):
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "64", "--height", "48", "--spp", "4", "--iterations", "5", "--threads", "4",
                          "--adaptive-pixels"] + list(flags), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_render_loop_stops_on_the_standard_error_in_the_middle_of_its_schedule(gpu):
    """64 x 48, five iterations.  A first run with a threshold of 0 (never met) prints the 95th percentile of the relative standard
    error after every iteration: it falls from each to the next.  A threshold between the second and the third value then stops the
    same run after iteration 3 -- neither the first nor the last.  The same threshold on the sample deviation is never met."""
    from statmc_amd import build
    build.build_tools()
    first = run_sim(build, "--stop-metric", "stderr", "--stop-at", "0.95:0")
    values = [float(v) for v in re.findall(r"Stop metric: iteration \d+, quantile 0.95 of the relative standard error = (\S+)", first)]
    assert len(values) == 5 and "Converged" not in first, first
    assert values[2] < min(values[:2]) and values[4] < values[2], values      # 8 -> 16 -> 64 samples per pixel on average
    threshold = 0.5 * (values[1] + values[2])
    second = run_sim(build, "--stop-metric", "stderr", "--stop-at", "0.95:%r" % threshold)
    m = re.findall(r"Converged: iteration (\d+), quantile 0.95 of the relative standard error = (\S+)", second)
    assert len(m) == 1 and int(m[0][0]) == 3 and float(m[0][1]) == values[2], second
    assert re.findall(r"Iteration: (\d+)", second) == ["1", "2", "3"]
    third = run_sim(build, "--stop-metric", "sd", "--stop-at", "0.95:%r" % threshold)
    assert "Converged" not in third and re.findall(r"Iteration: (\d+)", third) == ["1", "2", "3", "4", "5"]


def test_render_loop_plans_to_a_target_under_the_schedules_budget(gpu):
    from statmc_amd import build
    build.build_tools()
    W, H = 64, 48
    # a tolerance nobody reaches: every plan asks for more than the schedule has and falls back to the budget plan
    out = run_sim(build, "--target-error", "1e-6")
    plans = re.findall(r"Planned to target: total (\d+), need (\d+), n_open (\d+), n_capped (\d+), by (\w+)", out)
    spent = [int(s) for s in re.findall(r"Spent: (\d+) samples", out)]
    targets = [int(s) for s in re.findall(r"Target: (\d+) spp", out)]
    assert len(plans) == 4 and all(p[4] == "budget" and W * H * 0.9 < int(p[2]) <= W * H and p[2] == p[3] for p in plans), out
    assert spent == [W * H * t for t in targets] and len(re.findall(r"Planned: (\d+) samples", out)) == 4
    # a loose tolerance (the relative standard error of this source is about 0.3 at 4 samples per pixel): the plans run by the target,
    # spend less than the schedule, and fewer pixels are open at the last plan than at the first
    out = run_sim(build, "--target-error", "0.4", "--stop-metric", "stderr")
    plans = re.findall(r"Planned to target: total (\d+), need (\d+), n_open (\d+), n_capped (\d+), by (\w+)", out)
    spent = [int(s) for s in re.findall(r"Spent: (\d+) samples", out)]
    targets = [int(s) for s in re.findall(r"Target: (\d+) spp", out)]
    assert len(plans) == 4 and all(p[4] == "target" for p in plans), out
    assert spent[1:] == [int(p[0]) for p in plans] and all(s < W * H * t for s, t in zip(spent[1:], targets[1:]))
    opened = [int(p[2]) for p in plans]
    assert opened[0] > 0 and opened[-1] < opened[0], opened
    assert "Planned: " not in out


def test_without_the_new_flags_the_render_loop_prints_the_lines_it_printed(gpu):
    """The lines the existing tests parse, nothing else, in a run with --stop-at on the default metric: no line of the new flags."""
    from statmc_amd import build
    build.build_tools()
    out = run_sim(build, "--stop-at", "0.95:0")
    lines = out.splitlines()
    assert lines and all(line.startswith(SIM_LINES) for line in lines), out
    assert "Stop metric" not in out and "to target" not in out
    assert len(re.findall(r"Planned: (\d+) samples, (\d+) \.\. (\d+) per pixel, level 0x([0-9a-f]{8})", out)) == 4
    met = run_sim(build, "--stop-at", "0.95:1e30")
    assert re.findall(r"Converged: iteration 1, quantile 0.95 of the relative score = (\S+)", met) and "Iteration: 2" not in met
