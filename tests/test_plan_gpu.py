"""statmc_sample_scores / statmc_plan_samples on the device against the numpy float32 restatement of include/statmc.h
(tests/plan_reference.py, whose own properties tests/test_plan_cpu.py checks): scores and counts bit for bit, every field of the
result, determinism, a library stream, the loop statistics -> counts -> counted accumulation through FilmStats, the render loop's
--adaptive-pixels and the C++ Estimator.

One allowance, for NaN only: where the restatement's score is NaN the device's must be NaN, whichever sign and payload (the sign of
sqrt(-x) is the platform's: numpy on x86 gives -NaN, the device +NaN).  Every other score is held to the bit."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import plan_reference as ref
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
FILMS = [(37, 29), (64, 48), (257, 131)]     # odd with element tails; one aligned; several scan blocks and workgroups per candidate
FIELDS = ("total", "budget", "level_bits", "status", "n_live", "n_saturated")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_offset(a):
    """the same values in an image that starts 4 bytes into its allocation: 4-byte but not 16-byte aligned"""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    buf = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda:0")
    view = buf[1:1 + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(a.shape)


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.int32) if a.dtype == F32 else a


# ---------------------------------------------------------------- scores
def statistics(W, H, ch, seed):
    rng = np.random.default_rng(seed)
    special = np.array([0, 1, 2, 3, 4, 7, 100, 65536, (1 << 24) - 1, 1 << 24], np.int32)
    n = rng.integers(0, 300, (H, W)).astype(np.int32)
    pick = rng.random((H, W)) < 0.4
    n[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    mean = rng.normal(0, 2, (H, W, ch)).astype(F32)
    mean[rng.random(mean.shape) < 0.1] = 0
    m2 = (rng.lognormal(0, 2, (H, W, ch)) * np.maximum(n, 1)[..., None]).astype(F32)
    u = rng.random(m2.shape)
    m2[u < 0.10] = 0
    m2[(u >= 0.10) & (u < 0.13)] = -m2[(u >= 0.10) & (u < 0.13)]
    m2[(u >= 0.13) & (u < 0.15)] = np.nan
    m2[(u >= 0.15) & (u < 0.17)] = np.inf
    m2[(u >= 0.17) & (u < 0.19)] = F32(1e-42)       # subnormal sums and quotients
    mean[(u >= 0.19) & (u < 0.20)] = np.inf
    return n, mean, m2


def same_scores(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("metric", ["absolute", "relative"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_scores_equal_the_restatement_bit_for_bit(gpu, film, ch, metric):
    import torch
    W, H = film
    n, mean, m2 = statistics(W, H, ch, seed=W + ch)
    eps = 1e-3
    want = ref.scores_ref(n, mean, m2, gpu._METRICS[metric], eps)
    assert np.isinf(want).any() and np.isnan(want).any() and (want == 0).any() and (np.isfinite(want) & (want > 0)).sum() > W * H // 4
    got = gpu.sample_scores(dev(n), dev(mean if ch == 3 else mean[..., 0]), dev(m2 if ch == 3 else m2[..., 0]), metric=metric, eps=eps)
    torch.cuda.synchronize()
    same_scores(got.cpu().numpy(), want)
    # the element path: one plane 4 bytes off the 16-byte grid, same bits
    out = dev_offset(np.zeros((H, W), F32))
    gpu.sample_scores(dev(n), dev(mean), dev_offset(m2), metric=metric, eps=eps, out=out) if ch == 3 else \
        gpu.sample_scores(dev_offset(n), dev(mean[..., 0]), dev(m2[..., 0]), metric=metric, eps=eps, out=out)
    torch.cuda.synchronize()
    same_scores(out.cpu().numpy(), want)


# ---------------------------------------------------------------- plans
def next_up(x, k=1):
    return (np.array([x], F32).view(np.int32) + k).view(F32)[0]


def plan_cases(W, H):
    """name -> (score, n or None, budget, c_min, c_max); the restatement's plan is computed once per case (module cache below)"""
    rng = np.random.default_rng(W * 1000 + H)
    px = W * H
    logn = ref.lognormal_scores(H, W, seed=W)
    n40 = rng.integers(0, 40, (H, W)).astype(np.int32)
    cases = {}
    cases["lognormal"] = (logn, n40, px * 8, 1, 64)
    cases["lognormal_without_n"] = (logn, None, px * 8 + 5, 1, 64)
    cases["constant"] = (np.full((H, W), 0.75, F32), None, px * 10 + 37, 0, 1000)
    mixed = logn.copy().reshape(-1)
    kinds = rng.integers(0, 8, px)
    mixed[kinds == 0] = 0
    mixed[kinds == 1] = np.inf
    mixed[(kinds == 2) & (np.arange(px) % 2 == 0)] = np.nan
    mixed[(kinds == 2) & (np.arange(px) % 2 == 1)] = -3.5
    mixed[(kinds == 3) & (np.arange(px) % 3 == 0)] = F32(1e-30)
    mixed[(kinds == 3) & (np.arange(px) % 3 == 1)] = F32(3e37)
    cases["mixed_classes"] = (mixed.reshape(H, W), n40, px * 12, 2, 33)
    lo, hi = F32(2.0 ** -60), F32(2.0 ** 60)
    borders = np.array([lo, next_up(lo, -1), next_up(lo), hi, next_up(hi, -1), next_up(hi), F32(1), F32(2.5)], F32)
    cases["class_borders"] = (borders[rng.integers(0, len(borders), (H, W))], None, px * 3, 1, 9)
    big_n = np.array([0, 1, 1000, (1 << 24) - 1, 1 << 24, -5, (1 << 30) + 7, np.iinfo(np.int32).max], np.int32)[rng.integers(0, 8, (H, W))]
    cases["n_up_to_2_24_and_beyond"] = ((logn * F32(1e6)).astype(F32), big_n, px * 3000, 0, 1 << 20)
    cases["zero_to_one"] = (logn, n40, px // 3, 0, 1)
    cases["equal_bounds_floor"] = (logn, n40, px * 7, 7, 7)
    cases["equal_bounds_ceiling"] = (logn, n40, px * 7 + 1, 7, 7)
    cases["budget_is_a_T"] = (logn, n40, ref.total_at(0x40A00000, logn, n40, 1, 64), 1, 64)
    cases["budget_one_above_a_T"] = (logn, n40, ref.total_at(0x40A00000, logn, n40, 1, 64) + 1, 1, 64)
    floor, ceiling = ref.total_at(ref.U_LO, logn, n40, 1, 64), ref.total_at(ref.U_HI, logn, n40, 1, 64)
    cases["budget_at_the_floor"] = (logn, n40, floor, 1, 64)
    cases["budget_one_above_the_floor"] = (logn, n40, floor + 1, 1, 64)
    cases["budget_below_the_floor"] = (logn, n40, floor - 1, 1, 64)
    cases["budget_at_the_ceiling"] = (logn, n40, ceiling, 1, 64)
    cases["budget_above_the_ceiling"] = (logn, n40, ceiling + 1, 1, 64)
    cases["budget_zero"] = (logn, n40, 0, 1, 64)
    cases["budget_huge"] = (logn, None, 1 << 50, 0, 1 << 20)
    return cases


CASE_NAMES = sorted(plan_cases(8, 8))
_plans = {}


def planned(film, name):
    """the case and the restatement's (counts, result), computed once and left unchanged"""
    if (film, name) not in _plans:
        case = plan_cases(*film)[name]
        want = ref.plan_ref(*case)
        want[0].setflags(write=False)
        _plans[(film, name)] = (case, want)
    return _plans[(film, name)]


def run_plan(gpu, case, **kw):
    score, n, budget, c_min, c_max = case
    counts, res = gpu.plan_samples(dev(score), budget, c_min, c_max, n=None if n is None else dev(n), return_result=True, **kw)
    return counts.cpu().numpy(), res


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_plan_equals_the_restatement_bit_for_bit(gpu, film, name):
    case, (want, want_res) = planned(film, name)
    got, res = run_plan(gpu, case)
    assert {k: res[k] for k in FIELDS} == {k: want_res[k] for k in FIELDS}
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got.min() >= case[3] and got.max() <= case[4]
    if res["status"] == 0:
        assert int(got.astype(np.int64).sum()) == case[2] == res["total"]
    expected_status = {"budget_below_the_floor": 1, "budget_at_the_floor": 1, "budget_zero": 1, "equal_bounds_floor": 1, "budget_above_the_ceiling": 2,
                       "budget_huge": 2, "equal_bounds_ceiling": 2}
    assert res["status"] == expected_status.get(name, 0)


def test_unaligned_images_take_the_element_path_to_the_same_bits(gpu):
    import torch
    film = FILMS[2]
    (score, n, budget, c_min, c_max), (want, want_res) = planned(film, "mixed_classes")
    out = dev_offset(np.zeros(score.shape, np.int32))
    _, res = gpu.plan_samples(dev_offset(score), budget, c_min, c_max, n=dev_offset(n), out=out, return_result=True)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and {k: res[k] for k in FIELDS} == {k: want_res[k] for k in FIELDS}


def test_on_a_constant_film_the_first_pixels_in_raster_order_get_the_last_samples(gpu):
    film = FILMS[2]
    case, _ = planned(film, "constant")
    got, res = run_plan(gpu, case)
    q, extra = divmod(case[2], got.size)
    flat = got.reshape(-1)
    assert 0 < extra < got.size and np.all(flat[:extra] == q + 1) and np.all(flat[extra:] == q) and res["status"] == 0


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_same_bits_on_every_run_and_on_a_library_stream(gpu, film):
    import torch
    lib = gpu.load()
    case, (want, want_res) = planned(film, "mixed_classes")
    first, res1 = run_plan(gpu, case)
    second, res2 = run_plan(gpu, case)
    assert np.array_equal(first, second) and res1 == res2
    score, n, budget, c_min, c_max = case
    d_score, d_n = dev(score), dev(n)
    out = torch.full(score.shape, -1, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(gpu.plan_samples_workspace(*film), dtype=torch.uint8, device="cuda:0")
    result = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stream = C.c_void_p()
    gpu.check(lib.statmc_stream_create(C.byref(stream)))
    try:
        _, res3 = gpu.plan_samples(d_score, budget, c_min, c_max, n=d_n, out=out, workspace=ws, result=result, stream=stream, return_result=True)
    finally:
        gpu.check(lib.statmc_stream_destroy(stream))
    assert np.array_equal(out.cpu().numpy(), first) and res3 == res1


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(8, 8, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="c_min"):
        gpu.plan_samples(score, 10, 5, 4)
    with pytest.raises(gpu.StatmcError, match="budget"):
        gpu.plan_samples(score, -1, 0, 4)
    with pytest.raises(gpu.StatmcError, match="workspace_bytes"):
        gpu.plan_samples(score, 10, 0, 4, workspace=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(gpu.StatmcError, match="eps"):
        gpu.sample_scores(torch.ones(8, 8, dtype=torch.int32, device="cuda:0"), score, score.clone(), eps=0.0)


# ---------------------------------------------------------------- the loop: statistics -> counts -> counted accumulation
def test_film_stats_plans_what_its_counted_accumulation_takes(gpu):
    """8 spp, a plan of the next W H 8 samples, a capacity-16 arena accumulated with the planned counts: n grows by the counts at every
    pixel, and the moments are those of statmc_accumulate_records fed the same live samples (the counted entry's own contract)."""
    import torch
    from statmc_amd.film import STAT_TYPES, FilmStats
    W, H, CAP = 64, 48, 16
    names = ("radiance", "normal", "albedo")
    scene, smp, _ = make_case(W, H, 8)
    arena = {k: v.numpy() for k, v in scene.samples(CAP, seed=991, features=names).items()}
    d = torch.device("cuda:0")
    film, twin = FilmStats(W, H, d, types=names), FilmStats(W, H, d, types=names)
    for f in (film, twin):
        f.accumulate({t: dev(smp[t]) for t in names})
    counts, res = film.plan_samples(W * H * 8, 1, CAP, return_result=True)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (H, W)
    c = counts.cpu().numpy()
    assert res["status"] == 0 and res["total"] == W * H * 8 == int(c.sum()) and c.min() >= 1 and c.max() <= CAP and len(np.unique(c)) > 3
    rad = film.state["radiance"]
    score = ref.scores_ref(rad["n"].cpu().numpy(), rad["film_mean"].cpu().numpy(), rad["film_m2"].cpu().numpy(), ref.RELATIVE, 1e-3)
    want, want_res = ref.plan_ref(score, rad["n"].cpu().numpy(), W * H * 8, 1, CAP)
    assert np.array_equal(c, want) and {k: res[k] for k in FIELDS} == {k: want_res[k] for k in FIELDS}
    n_before = rad["n"].cpu().numpy().copy()
    film.accumulate({t: dev(arena[t]) for t in names}, counts=counts)
    torch.cuda.synchronize()
    assert np.array_equal(film.state["radiance"]["n"].cpu().numpy() - n_before, c)
    live = (np.arange(CAP)[:, None] < c.reshape(-1)[None, :]).T                     # [npx, CAP]
    pixels = dev(np.repeat(np.arange(W * H, dtype=np.int32), c.reshape(-1)))
    recs = [dev(np.ascontiguousarray(arena[t].reshape(CAP, W * H, -1).transpose(1, 0, 2)[live])) for t in names]
    sts = [gpu.make_stat_type_records(recs[i], STAT_TYPES[t]["channels"], twin.state[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"])
           for i, t in enumerate(names)]
    gpu.accumulate_records(W, H, sts, pixels)
    torch.cuda.synchronize()
    for t in names:
        for k, v in film.state[t].items():
            if v is not None:
                assert np.array_equal(bits(v), bits(twin.state[t][k])), (t, k)


def test_render_loop_plans_per_pixel(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels: 96 x 56, three iterations.  Every printed plan spends the next iteration's W H target
    samples exactly, the dumped n sums to the whole schedule, and n differs between pixels."""
    from statmc_amd import build, pfm
    build.build_tools()
    W, H = 96, 56
    stem = str(tmp_path / "sim")
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", str(W), "--height", str(H), "--spp", "4", "--iterations", "3", "--threads", "4",
                          "--adaptive-pixels", "--stem", stem], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    spent = [int(m) for m in re.findall(r"Spent: (\d+) samples", out.stdout)]
    plans = re.findall(r"Planned: (\d+) samples, (\d+) \.\. (\d+) per pixel, level 0x([0-9a-f]{8})", out.stdout)
    targets = [int(m) for m in re.findall(r"Target: (\d+) spp", out.stdout)]
    assert len(targets) == 3 and len(spent) == 3 and len(plans) == 2, out.stdout
    assert spent == [W * H * t for t in targets]
    for (total, lo, hi, level), t in zip(plans, targets[1:]):
        assert int(total) == W * H * t and 1 <= int(lo) < int(hi) <= 4 * t
        assert ref.U_LO <= int(level, 16) <= ref.U_HI
    assert targets == [4, 4, 8]
    n = np.asarray(pfm.read_pfm("%s-%d-t0-b0-n.pfm" % (stem, sum(targets))))
    assert int(n.astype(np.int64).sum()) == sum(spent) and n.min() != n.max()
    assert np.array_equal(n, np.asarray(pfm.read_pfm("%s-%d-t1-b0-n.pfm" % (stem, sum(targets)))))     # every type got the same counts


def test_estimator_plans_what_the_python_entry_plans(gpu, tmp_path):
    """C++ host: Estimator::PlanSamples followed by AccumulateFilm(S, buffers, d_counts) on a small film; the count image and result it
    dumps equal the Python entry's for the statistics it dumps (tests/cpp/test_plan_samples.cpp)."""
    import torch
    from statmc_amd import build
    build.build_tools()
    W, H, CAP = 61, 37, 12
    prefix = str(tmp_path / "plan")
    out = subprocess.run([build.PLAN_BIN, str(W), str(H), str(CAP), prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan samples ok" in out.stdout
    n = np.fromfile(prefix + ".n.i32", np.int32).reshape(H, W)
    mean = np.fromfile(prefix + ".film_mean.f32", F32).reshape(H, W, 3)
    m2 = np.fromfile(prefix + ".film_m2.f32", F32).reshape(H, W, 3)
    counts = np.fromfile(prefix + ".counts.i32", np.int32).reshape(H, W)
    m = re.search(r"result: total (\d+) budget (\d+) level 0x([0-9a-f]{8}) status (\d+) live (\d+) saturated (\d+)", out.stdout)
    score = gpu.sample_scores(dev(n), dev(mean), dev(m2), metric="relative", eps=1e-3)
    got, res = gpu.plan_samples(score, int(m.group(2)), 1, CAP, n=dev(n), return_result=True)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), counts) and len(np.unique(counts)) > 2
    assert [res[k] for k in FIELDS] == [int(m.group(1)), int(m.group(2)), int(m.group(3), 16), int(m.group(4)), int(m.group(5)), int(m.group(6))]
