"""statmc_score_window on the device against the numpy restatement of include/statmc.h (tests/score_window_reference.py, whose own
properties tests/test_score_window_cpu.py checks): every pixel bit for bit, no tolerance anywhere; unaligned images, containment,
determinism, a library stream, composition, max_pool2d, the classes statmc_score_select assigns, the refusals, and the upper layers:
FilmStats' dilate, the C++ Estimator's scoreDilate / ScoreWindow and the render loop's --score-dilate."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import score_window_reference as ref
import select_reference as sel
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
# smaller than the radius; one row; one column; a few pixels; one tile row of two tiles; one past a tile edge in x, one short in y;
# several tiles with ragged last tiles, twice
FILMS = [(1, 1), (67, 1), (1, 67), (5, 3), (64, 64), (65, 63), (130, 70), (257, 131)]
RADII = [0, 1, 2, 7, 20, 32]
OPS = [ref.MAX, ref.MIN]
OP_NAMES = {ref.MAX: "max", ref.MIN: "min"}
SENTINEL = F32(-12345.0)
GUARD = 64


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_offset(a, floats=1):
    """the same values in an image that starts `floats` floats into its allocation: 4-byte but not 16-byte aligned"""
    import torch
    flat = torch.from_numpy(np.array(a, order="C").reshape(-1)).cuda()
    buf = torch.zeros(flat.numel() + 8, dtype=flat.dtype, device="cuda:0")
    view = buf[floats:floats + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4 * floats
    return view.view(a.shape)


def host_bits(t):
    import torch
    torch.cuda.synchronize()
    return ref.bits(t.cpu().numpy())


_wanted = {}


def wanted(film, name, op, radius):
    """(score image, the restatement's window), computed once and left unchanged"""
    key = (film, name, op, radius)
    if key not in _wanted:
        score = ref.image(name, *film)
        out = ref.window_ref(score, op, radius)
        score.setflags(write=False)
        out.setflags(write=False)
        _wanted[key] = (score, out)
    return _wanted[key]


# ---------------------------------------------------------------- 1. the entry against the restatement
@pytest.mark.parametrize("name", ref.IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_window_equals_the_restatement_bit_for_bit(gpu, film, name):
    d_score = dev(ref.image(name, *film))
    for op in OPS:
        for r in RADII:
            score, want = wanted(film, name, op, r)
            got = gpu.score_window(d_score, r, OP_NAMES[op])
            bad = np.argwhere(host_bits(got) != ref.bits(want))
            assert bad.size == 0, (OP_NAMES[op], r, len(bad), bad[:4].tolist())
    assert np.array_equal(host_bits(d_score), ref.bits(score))      # score is only read
    if name == "constant":
        assert np.all(host_bits(got) == 0x3F400000)


@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_a_1280x720_film_at_radius_20(gpu, op):
    film = (1280, 720)
    score, want = wanted(film, "mixed_classes", op, 20)
    assert np.array_equal(host_bits(gpu.score_window(dev(score), 20, OP_NAMES[op])), ref.bits(want))


@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
@pytest.mark.parametrize("film", [(5, 3), (65, 63), (130, 70)], ids=lambda f: "%dx%d" % f)
def test_an_impulse_becomes_exactly_the_clipped_square(gpu, film, op):
    w, h = film
    for site in ref.impulse_sites(w, h):
        d_score = dev(ref.impulse(w, h, site, op))
        for r in (1, 7, 32):
            got = host_bits(gpu.score_window(d_score, r, OP_NAMES[op]))
            assert np.array_equal(got, ref.bits(ref.impulse_answer(w, h, site, op, r))), (site, r)


@pytest.mark.parametrize("film", [(67, 1), (5, 3), (65, 63), (257, 131)], ids=lambda f: "%dx%d" % f)
def test_unaligned_pointers_take_the_element_path_to_the_same_bits(gpu, film):
    import torch
    for op in OPS:
        for r in (1, 20):
            score, want = wanted(film, "mixed_classes", op, r)
            for score_off, out_off in ((1, 0), (0, 1), (1, 1), (3, 2)):
                d_score = dev_offset(score, score_off) if score_off else dev(score)
                buf = torch.zeros(score.size + 8, dtype=torch.float32, device="cuda:0")
                out = buf[out_off:out_off + score.size].view(score.shape)
                assert out.data_ptr() % 16 == 4 * out_off
                gpu.score_window(d_score, r, OP_NAMES[op], out=out)
                assert np.array_equal(host_bits(out), ref.bits(want)), (OP_NAMES[op], r, score_off, out_off)


@pytest.mark.parametrize("film", [(1, 1), (5, 3), (65, 63), (257, 131)], ids=lambda f: "%dx%d" % f)
def test_only_out_is_written(gpu, film):
    """out pre-filled with a sentinel inside an allocation with 64 sentinel floats before and after it: exactly width * height
    floats change; score does not."""
    import torch
    px = film[0] * film[1]
    for op in OPS:
        for r, out_off in ((0, 0), (7, 0), (32, 1)):
            score, want = wanted(film, "mixed_classes", op, r)
            d_score = dev(score)
            buf = torch.full((GUARD + out_off + px + GUARD + 4,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
            out = buf[GUARD + out_off:GUARD + out_off + px].view(score.shape)
            gpu.score_window(d_score, r, OP_NAMES[op], out=out)
            whole = host_bits(buf)
            assert np.array_equal(whole[GUARD + out_off:GUARD + out_off + px].reshape(score.shape), ref.bits(want)), (OP_NAMES[op], r)
            assert np.all(whole[:GUARD + out_off] == ref.bits(SENTINEL)) and np.all(whole[GUARD + out_off + px:] == ref.bits(SENTINEL)), (OP_NAMES[op], r)
            assert np.array_equal(host_bits(d_score), ref.bits(score))


@pytest.mark.parametrize("film", [(65, 63), (257, 131)], ids=lambda f: "%dx%d" % f)
def test_two_runs_and_a_library_stream_give_the_same_bits(gpu, film):
    import torch
    lib = gpu.load()
    for op in OPS:
        score, want = wanted(film, "mixed_classes", op, 7)
        d_score = dev(score)
        first = host_bits(gpu.score_window(d_score, 7, OP_NAMES[op]))
        second = host_bits(gpu.score_window(d_score, 7, OP_NAMES[op]))
        assert np.array_equal(first, second) and np.array_equal(first, ref.bits(want))
        out = torch.full(score.shape, float(SENTINEL), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        stream = C.c_void_p()
        gpu.check(lib.statmc_stream_create(C.byref(stream)))
        try:
            t = gpu.score_window(d_score, 7, OP_NAMES[op], out=out, stream=stream)
            gpu.check(lib.statmc_synchronize(stream))
        finally:
            gpu.check(lib.statmc_stream_destroy(stream))
        assert t.data_ptr() == out.data_ptr() and np.array_equal(host_bits(t), first)


@pytest.mark.parametrize("film", [(65, 63), (257, 131)], ids=lambda f: "%dx%d" % f)
def test_windows_compose_on_the_device(gpu, film):
    for op in OPS:
        for r1, r2 in ((7, 13), (20, 12)):
            score, want = wanted(film, "mixed_classes", op, r1 + r2)
            twice = gpu.score_window(gpu.score_window(dev(score), r1, OP_NAMES[op]), r2, OP_NAMES[op])
            once = gpu.score_window(dev(score), r1 + r2, OP_NAMES[op])
            assert np.array_equal(host_bits(twice), host_bits(once)) and np.array_equal(host_bits(once), ref.bits(want)), (OP_NAMES[op], r1, r2)


@pytest.mark.parametrize("film", [(5, 3), (130, 70), (257, 131)], ids=lambda f: "%dx%d" % f)
def test_max_is_max_pool2d_on_the_device(gpu, film):
    import torch
    for name in ("lognormal", "mixed_classes"):
        canon = gpu.score_window(dev(ref.image(name, *film)), 0, "max")      # non-negative, no NaN
        for r in RADII:
            pooled = torch.nn.functional.max_pool2d(canon[None, None], kernel_size=2 * r + 1, stride=1, padding=r)[0, 0]
            assert np.array_equal(host_bits(pooled), host_bits(gpu.score_window(canon, r, "max"))), (name, r)


@pytest.mark.parametrize("op", OPS, ids=OP_NAMES.get)
def test_the_classes_of_the_windowed_image_are_the_restatements(gpu, op):
    film = (257, 131)
    for r in (0, 2, 20):
        score, want = wanted(film, "mixed_classes", op, r)
        got = gpu.read_select_result(gpu.score_select(gpu.score_window(dev(score), r, OP_NAMES[op]), [0]))
        live, sat = sel.class_counts(sel.keys_of(want))
        assert (got["n_live"], got["n_saturated"]) == (live, sat), r
        if r == 0:      # every class is there before a wide window floods the film with +inf (MAX) or 0 (MIN)
            assert 0 < live < score.size and sat > 0


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(8, 8, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="radius = 33"):
        gpu.score_window(score, 33)
    with pytest.raises(gpu.StatmcError, match="radius = -1"):
        gpu.score_window(score, -1)
    with pytest.raises(gpu.StatmcError, match="op = 2"):
        gpu.score_window(score, 1, op=2)
    with pytest.raises(gpu.StatmcError, match="out overlaps score"):
        gpu.score_window(score, 1, out=score)
    both = torch.ones(2 * 64 - 1, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="out overlaps score"):
        gpu.score_window(both[:64].view(8, 8), 1, out=both[63:].view(8, 8))
    with pytest.raises(ValueError):
        gpu.score_window(score, 1, out=torch.ones(8, 7, device="cuda:0"))
    with pytest.raises(KeyError):
        gpu.score_window(score, 1, op="mean")


# ---------------------------------------------------------------- 2. the upper layers
def test_film_stats_dilate(gpu, monkeypatch):
    """8 spp accumulated into a FilmStats: plan_samples(dilate=3) is the plan of the windowed score image and sums to the budget;
    score_quantiles / score_count_above with dilate read the same image; dilate=0 makes the calls it made before, no window."""
    import torch
    from statmc_amd.film import FilmStats
    W, H = 64, 48
    names = ("radiance", "normal", "albedo")
    _, smp, _ = make_case(W, H, 8)
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names})
    rad = film.state["radiance"]
    scores = gpu.sample_scores(rad["n"], rad["film_mean"], rad["film_m2"], metric="relative", eps=1e-3)
    budget = W * H * 4
    windowed = gpu.score_window(scores, 3)
    want = gpu.plan_samples(windowed, budget, 1, 16, n=rad["n"])
    got, res = film.plan_samples(budget, 1, 16, dilate=3, return_result=True)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and int(got.sum()) == budget and res["status"] == 0 and res["total"] == budget
    plain = film.plan_samples(budget, 1, 16)
    assert torch.equal(plain, gpu.plan_samples(scores, budget, 1, 16, n=rad["n"])) and not torch.equal(plain, got)
    host = ref.window_ref(scores.cpu().numpy(), ref.MAX, 3)
    assert np.array_equal(host_bits(windowed), ref.bits(host))
    ranks = [sel.nearest_rank(q, W * H) for q in (0.5, 0.95)]
    assert np.array_equal(film.score_quantiles([0.5, 0.95], dilate=3).view(np.uint32), np.array(sel.select_ref(host, ranks)["value_bits"], np.uint32))
    th = [0.0, float(np.median(host))]
    assert film.score_count_above(th, dilate=3) == sel.count_above_ref(host, th)
    # dilate = 0: the calls of before, in their order, and never the window
    calls = []
    for fn in ("sample_scores", "score_window", "plan_samples", "score_select", "score_count_above"):
        monkeypatch.setattr(gpu, fn, (lambda name, real: lambda *a, **k: (calls.append(name), real(*a, **k))[1])(fn, getattr(gpu, fn)))
    film.plan_samples(budget, 1, 16, dilate=0)
    film.score_quantiles([0.5], dilate=0)
    film.score_count_above([0.0])
    assert calls == ["sample_scores", "plan_samples", "sample_scores", "score_select", "sample_scores", "score_count_above"]
    del calls[:]
    film.plan_samples(budget, 1, 16, dilate=2)
    assert calls == ["sample_scores", "score_window", "plan_samples"]


def test_estimator_plans_what_the_python_entries_plan(gpu, tmp_path):
    """C++ host (tests/cpp/test_score_window.cpp): Estimator::PlanSamples(..., scoreDilate) gives the counts of api.plan_samples on
    api.score_window of the scores of the statistics it dumps; scoreDilate = 0 counts score images as before; Estimator::ScoreWindow on
    a caller's image is the restatement's erosion and opening."""
    import torch
    from statmc_amd import build
    build.build_tools()
    W, H, DILATE = 61, 37, 3
    prefix = str(tmp_path / "window")
    out = subprocess.run([build.WINDOW_BIN, str(W), str(H), str(DILATE), prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "score window ok" in out.stdout
    n = np.fromfile(prefix + ".n.i32", np.int32).reshape(H, W)
    mean = np.fromfile(prefix + ".film_mean.f32", F32).reshape(H, W, 3)
    m2 = np.fromfile(prefix + ".film_m2.f32", F32).reshape(H, W, 3)
    d_n = dev(n)
    scores = gpu.sample_scores(d_n, dev(mean), dev(m2), metric="relative", eps=1e-3)
    budget = W * H * 4
    for name, radius in (("counts0", 0), ("counts", DILATE)):
        got = np.fromfile("%s.%s.i32" % (prefix, name), np.int32).reshape(H, W)
        want, res = gpu.plan_samples(gpu.score_window(scores, radius) if radius else scores, budget, 1, 8, n=d_n, return_result=True)
        assert np.array_equal(got, want.cpu().numpy()) and int(got.sum()) == budget, name
        assert "plan: dilate %d total %d status 0 level 0x%08x" % (radius, budget, res["level_bits"]) in out.stdout
    own = np.fromfile(prefix + ".own.f32", F32).reshape(H, W)
    eroded = ref.window_ref(own, ref.MIN, 2)
    assert np.array_equal(ref.bits(np.fromfile(prefix + ".eroded.f32", F32).reshape(H, W)), ref.bits(eroded))
    assert np.array_equal(ref.bits(np.fromfile(prefix + ".opened.f32", F32).reshape(H, W)), ref.bits(ref.window_ref(eroded, ref.MAX, 2)))
    assert own.max() == F32(1e6) and eroded.max() < 3


def run_sim(build, stem, *extra):
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "96", "--height", "64", "--spp", "4", "--iterations", "3", "--threads", "4",
                          "--adaptive-pixels", "--stem", stem] + list(extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_render_loop_plans_by_the_dilated_score(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels --score-dilate 2 on 96 x 64, three iterations: every plan spends its budget to the sample,
    the sample counts it leaves differ from the run without the flag, and --score-dilate 0 is that run byte for byte."""
    from statmc_amd import build
    build.build_tools()
    plain, zero, dilated = (str(tmp_path / s) for s in ("plain", "zero", "dilated"))
    out_plain = run_sim(build, plain)
    out_zero = run_sim(build, zero, "--score-dilate", "0")
    out_dilated = run_sim(build, dilated, "--score-dilate", "2", "--stop-at", "0.95:0")
    for text in (out_plain, out_dilated):
        planned = [int(t) for t in re.findall(r"^Planned: (\d+) samples", text, re.M)]
        assert planned == [96 * 64 * 4, 96 * 64 * 8], text      # iterations 2 and 3: the schedule's targets, to the sample
    assert "Converged" not in out_dilated
    dumps = lambda stem: {os.path.basename(p)[len(os.path.basename(stem)):]: open(p, "rb").read() for p in sorted(glob.glob(stem + "-*.pfm"))}
    d_plain, d_zero, d_dilated = dumps(plain), dumps(zero), dumps(dilated)
    assert len(d_plain) > 10 and d_plain == d_zero and sorted(d_plain) == sorted(d_dilated)
    last_n = [k for k in d_plain if re.search(r"-t0-b0-n\.pfm$", k)]
    assert last_n and any(d_plain[k] != d_dilated[k] for k in last_n)
    # the flag without --adaptive-pixels, and malformed ones
    for bad in (["--score-dilate", "2"], ["--adaptive-pixels", "--score-dilate", "33"], ["--adaptive-pixels", "--score-dilate", "x"]):
        r = subprocess.run([build.RENDER_SIM_BIN, "--width", "16", "--height", "16"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--score-dilate" in r.stderr, bad
