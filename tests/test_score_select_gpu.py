"""statmc_score_select / statmc_score_count_above on the device against the numpy restatement of include/statmc.h
(tests/select_reference.py, whose own properties tests/test_score_select_cpu.py checks): every field of the result bit for bit, no
tolerance anywhere; unaligned images, a workspace full of garbage, determinism, a library stream, the classes of
statmc_plan_samples, the two entries tied to each other, FilmStats.score_quantiles, the C++ Estimator and the render loop's
--stop-at."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import plan_reference as plan_ref
import select_reference as ref
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
# one pixel; three (one partial quad); odd with element tails; aligned; several workgroups; 900 chunks of 1024 pixels for a pass
# grid capped at 768: the stride loop runs twice in the first 132 workgroups
FILMS = [(1, 1), (3, 1), (37, 29), (64, 48), (257, 131), (1280, 720)]
IMAGES = ["lognormal", "constant", "two_values", "mixed_classes", "class_borders", "low_byte_only", "top_byte_only", "all_nan", "all_inf"]
TWO_LOW, TWO_HIGH = F32(0.25), F32(3.0)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_offset(a):
    """the same values in an image that starts 4 bytes into its allocation: 4-byte but not 16-byte aligned (as tests/test_plan_gpu.py
    makes it)"""
    import torch
    flat = torch.from_numpy(np.array(a, order="C").reshape(-1)).cuda()
    buf = torch.zeros(flat.numel() + 4, dtype=flat.dtype, device="cuda:0")
    view = buf[1:1 + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(a.shape)


def from_bits(b):
    return np.asarray(b, np.uint32).view(F32)


def image(name, W, H):
    rng = np.random.default_rng(W * 1000 + H + IMAGES.index(name))
    px = W * H
    logn = plan_ref.lognormal_scores(H, W, seed=W)
    if name == "lognormal":
        return logn
    if name == "constant":                  # one bin in every pass
        return np.full((H, W), 0.75, F32)
    if name == "two_values":                # the first `step` pixels in raster order are the low value
        s = np.full(px, TWO_HIGH, F32)
        s[:two_values_step(px)] = TWO_LOW
        return s.reshape(H, W)
    if name == "mixed_classes":             # the plan tests' mixed classes, and -0, -inf and NaN of both signs
        mixed = logn.copy().reshape(-1)
        kinds = rng.integers(0, 10, px)
        at = np.arange(px)
        mixed[kinds == 0] = 0
        mixed[kinds == 1] = np.inf
        mixed[(kinds == 2) & (at % 2 == 0)] = np.nan
        mixed[(kinds == 2) & (at % 2 == 1)] = -3.5
        mixed[(kinds == 3) & (at % 3 == 0)] = F32(1e-30)
        mixed[(kinds == 3) & (at % 3 == 1)] = F32(3e37)
        mixed[kinds == 4] = F32(1e-42)
        mixed[(kinds == 5) & (at % 3 == 0)] = -0.0
        mixed[(kinds == 5) & (at % 3 == 1)] = -np.inf
        bits = mixed.view(np.uint32)
        bits[(kinds == 5) & (at % 3 == 2)] = 0xFFC00001      # a NaN with the sign bit
        return mixed.reshape(H, W)
    if name == "class_borders":             # 2^-60 and 2^60, one bit pattern up and down, and two live values
        b = np.array([ref.LIVE_LO, ref.LIVE_LO - 1, ref.LIVE_LO + 1, ref.LIVE_HI, ref.LIVE_HI - 1, ref.LIVE_HI + 1, 0x3F800000, 0x40200000], np.uint32)
        return from_bits(b[rng.integers(0, len(b), (H, W))])
    if name == "low_byte_only":             # only the last pass separates them
        return from_bits(np.uint32(0x3F801200) + rng.integers(0, 256, (H, W)).astype(np.uint32))
    if name == "top_byte_only":             # pass 0 settles it: 2^-126 ... 2^126 in steps of the top byte
        return from_bits((rng.integers(0, 0x7F, (H, W)).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00345678))
    if name == "all_nan":
        return np.full((H, W), np.nan, F32)
    if name == "all_inf":
        return np.full((H, W), np.inf, F32)
    raise KeyError(name)


def two_values_step(px):
    return max(px * 3 // 8, 1) if px > 1 else 1


def rank_sets(name, px):
    """0, P - 1 and P // 2; eight at once, unsorted, one repeated; one alone; on one pixel rank 0 eight times"""
    rng = np.random.default_rng(px)
    eight = [int(r) for r in rng.integers(0, px, 7)]
    eight.insert(5, eight[1])
    sets = [[0, px - 1, px // 2], eight, [px * 2 // 3]]
    if px == 1:
        sets.append([0] * 8)
    if name == "two_values":                # a rank on each side of the step and exactly at it
        step = two_values_step(px)
        sets.append(sorted({max(step - 1, 0), min(step, px - 1), min(step + 1, px - 1)}, reverse=True))
    return sets


_cases = {}


def case(film, name):
    """(score image, {ranks: the restatement's result}), computed once and left unchanged"""
    if (film, name) not in _cases:
        W, H = film
        score = image(name, W, H)
        score.setflags(write=False)
        want = {tuple(r): ref.select_ref(score, r) for r in rank_sets(name, W * H)}
        _cases[(film, name)] = (score, want)
    return _cases[(film, name)]


def select(gpu, d_score, ranks, **kw):
    import torch
    res = gpu.score_select(d_score, ranks, **kw)
    if "stream" not in kw:
        torch.cuda.synchronize()
    return res


def fields(d):
    return {k: d[k] for k in ref.FIELDS}


def whole_struct(gpu, t):
    """the 256 bytes as the device wrote them, the slots behind n_ranks and the pad included"""
    r = gpu.SelectResult.from_buffer_copy(t.cpu().numpy().tobytes())
    return [int(r.n_px), int(r.n_live), int(r.n_saturated), int(r.n_ranks), int(r.pad)] + [int(v) for f in ("rank", "value_bits", "n_below", "n_equal")
                                                                                            for v in getattr(r, f)]


@pytest.mark.parametrize("name", IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_select_equals_the_restatement_bit_for_bit(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    for ranks, w in want.items():
        t = select(gpu, d_score, list(ranks))
        got = gpu.read_select_result(t)
        assert fields(got) == w, (ranks, fields(got), w)
        assert np.array_equal(got["values"].view(np.uint32), np.array(w["value_bits"], np.uint32))
        raw = whole_struct(gpu, t)
        k = len(ranks)
        for j in range(4):      # slots n_ranks .. 7 of the four arrays are written as 0
            assert raw[5 + 8 * j + k:5 + 8 * j + 8] == [0] * (8 - k), (ranks, j)
        assert raw[4] == 0
        for i, r in enumerate(ranks):
            assert got["n_below"][i] <= r < got["n_below"][i] + got["n_equal"][i]
    px = film[0] * film[1]
    first = want[(0, px - 1, px // 2)]
    if name in ("constant", "all_inf", "all_nan"):
        assert first["n_equal"] == [px] * 3 and first["n_below"] == [0] * 3
        assert first["value_bits"] == [{"constant": 0x3F400000, "all_inf": 0x7F800000, "all_nan": 0}[name]] * 3
    if name == "two_values" and px > 3:
        step = two_values_step(px)
        w = want[tuple(sorted({step - 1, step, step + 1}, reverse=True))]
        assert w["value_bits"] == [0x40400000, 0x40400000, 0x3E800000] and w["n_below"] == [step, step, 0] and w["n_equal"] == [px - step, px - step, step]


def thresholds_of(score):
    """0, -1, +inf, 1e-42, a value present in the image, its neighbours one pattern up and down (inside [+0, +inf]: beyond lie -0's
    and NaN's patterns, which are other keys or refused), 2^60"""
    present = int(ref.select_ref(score, [score.size // 2])["value_bits"][0])
    return [F32(0), F32(-1), F32(np.inf), F32(1e-42), from_bits([present])[0], from_bits([min(present + 1, 0x7F800000)])[0],
            from_bits([max(present - 1, 0)])[0], F32(2.0 ** 60)]


@pytest.mark.parametrize("name", IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_count_above_equals_the_restatement_and_the_select(gpu, film, name):
    import torch
    score, _ = case(film, name)
    th = thresholds_of(score)
    want = ref.count_above_ref(score, th)
    d_score = dev(score)
    got = gpu.score_count_above(d_score, th)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and [int(c) for c in got.cpu().numpy()] == want
    # the count above a value the select returned is what the select leaves above it
    sel = gpu.read_select_result(select(gpu, d_score, [score.size // 2]))
    assert sel["value_bits"][0] == ref.key_of(th[4])
    assert want[4] == sel["n_px"] - sel["n_below"][0] - sel["n_equal"][0]
    assert want[1] == want[0] and want[2] == 0      # a negative threshold is +0's key; nothing is above +inf
    one = gpu.score_count_above(d_score, [th[4]])     # one threshold alone
    out = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    gpu.score_count_above(dev_offset(score), th, out=out)      # the element path, the caller's counts
    torch.cuda.synchronize()
    assert [int(c) for c in one.cpu().numpy()] == [want[4]] and [int(c) for c in out.cpu().numpy()] == want


@pytest.mark.parametrize("name", ["lognormal", "mixed_classes", "constant"])
@pytest.mark.parametrize("film", [(3, 1), (37, 29), (257, 131), (1280, 720)], ids=lambda f: "%dx%d" % f)
def test_unaligned_images_take_the_element_path_to_the_same_bits(gpu, film, name):
    score, want = case(film, name)
    d_score = dev_offset(score)
    for ranks, w in want.items():
        assert fields(gpu.read_select_result(select(gpu, d_score, list(ranks)))) == w, ranks


@pytest.mark.parametrize("film", [(37, 29), (257, 131), (1280, 720)], ids=lambda f: "%dx%d" % f)
def test_a_workspace_full_of_garbage_two_runs_and_a_library_stream_give_the_same_bits(gpu, film):
    import torch
    lib = gpu.load()
    score, want = case(film, "mixed_classes")
    ranks = [r for r in want if len(r) == 8][0]
    d_score = dev(score)
    first = whole_struct(gpu, select(gpu, d_score, list(ranks)))
    second = whole_struct(gpu, select(gpu, d_score, list(ranks)))
    assert first == second and fields(gpu.read_select_result(select(gpu, d_score, list(ranks)))) == want[ranks]
    ws = torch.full((gpu.score_select_workspace(),), 0xFF, dtype=torch.uint8, device="cuda:0")
    result = torch.full((32,), -1, dtype=torch.int64, device="cuda:0")
    assert whole_struct(gpu, select(gpu, d_score, list(ranks), workspace=ws, result=result)) == first
    ws.fill_(0xFF)
    result.fill_(-1)
    torch.cuda.synchronize()
    stream = C.c_void_p()
    gpu.check(lib.statmc_stream_create(C.byref(stream)))
    try:
        t = gpu.score_select(d_score, list(ranks), workspace=ws, result=result, stream=stream)
        counts = gpu.score_count_above(d_score, [0.5, 2.0], stream=stream)
        gpu.check(lib.statmc_synchronize(stream))
    finally:
        gpu.check(lib.statmc_stream_destroy(stream))
    assert t.data_ptr() == result.data_ptr() and whole_struct(gpu, t) == first
    assert [int(c) for c in counts.cpu().numpy()] == ref.count_above_ref(score, [0.5, 2.0])


@pytest.mark.parametrize("name", ["lognormal", "mixed_classes", "class_borders", "all_nan", "all_inf"])
def test_the_classes_are_those_of_plan_samples(gpu, name):
    film = FILMS[4]
    score, want = case(film, name)
    d_score = dev(score)
    _, plan = gpu.plan_samples(d_score, score.size * 4, 0, 8, return_result=True)
    sel = gpu.read_select_result(select(gpu, d_score, [0]))
    assert (sel["n_live"], sel["n_saturated"]) == (plan["n_live"], plan["n_saturated"])
    live, sat = plan_ref.classes(score)
    assert (sel["n_live"], sel["n_saturated"]) == (int(live.sum()), int(sat.sum()))
    if name in ("mixed_classes", "class_borders"):
        assert 0 < sel["n_live"] < score.size and sel["n_saturated"] > 0


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(8, 8, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="n_ranks"):
        gpu.score_select(score, [])
    with pytest.raises(gpu.StatmcError, match="n_ranks"):
        gpu.score_select(score, list(range(9)))
    with pytest.raises(gpu.StatmcError, match=r"ranks\[1\]"):
        gpu.score_select(score, [0, 64])
    with pytest.raises(gpu.StatmcError, match="workspace_bytes"):
        gpu.score_select(score, [0], workspace=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(gpu.StatmcError, match="result overlaps score"):
        gpu.score_select(score, [0], result=score.view(torch.int64))
    with pytest.raises(gpu.StatmcError, match="NaN"):
        gpu.score_count_above(score, [1.0, float("nan")])
    with pytest.raises(gpu.StatmcError, match="n_thresholds"):
        gpu.score_count_above(score, [1.0] * 9, out=torch.zeros(9, dtype=torch.int64, device="cuda:0"))


# ---------------------------------------------------------------- the upper layers
def test_film_stats_score_quantiles_and_counts(gpu):
    """8 spp accumulated into a FilmStats; the quantiles of its relative radiance score are the restatement's on the downloaded score
    image, at the nearest ranks."""
    import torch
    from statmc_amd.film import FilmStats
    W, H = 64, 48
    names = ("radiance", "normal", "albedo")
    _, smp, _ = make_case(W, H, 8)
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names})
    qs = [0, 0.5, 0.95, 1]
    for metric in ("relative", "absolute"):
        got = film.score_quantiles(qs, metric=metric)
        rad = film.state["radiance"]
        score = gpu.sample_scores(rad["n"], rad["film_mean"], rad["film_m2"], metric=metric, eps=1e-3).cpu().numpy()
        ranks = [ref.nearest_rank(q, W * H) for q in qs]
        assert ranks == [0, 1535, 2918, 3071]
        want = ref.select_ref(score, ranks)
        assert got.dtype == F32 and np.array_equal(got.view(np.uint32), np.array(want["value_bits"], np.uint32))
        assert got[0] <= got[1] <= got[2] <= got[3] and got[1] > 0
        th = [0.0, float(got[1]), float(got[2]), 1e30]
        assert film.score_count_above(th, metric=metric) == ref.count_above_ref(score, th)
    with pytest.raises(ValueError):
        film.score_quantiles([1.5])


def test_estimator_selects_what_the_python_entry_selects(gpu, tmp_path):
    """C++ host: Estimator::ScoreSelect / ScoreCountAbove on a small film, the score image shared with PlanSamples
    (tests/cpp/test_score_select.cpp); what it prints equals the restatement on the scores of the statistics it dumps."""
    from statmc_amd import build
    build.build_tools()
    W, H = 61, 37
    prefix = str(tmp_path / "select")
    out = subprocess.run([build.SELECT_BIN, str(W), str(H), prefix], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "score select ok" in out.stdout
    n = np.fromfile(prefix + ".n.i32", np.int32).reshape(H, W)
    mean = np.fromfile(prefix + ".film_mean.f32", F32).reshape(H, W, 3)
    m2 = np.fromfile(prefix + ".film_m2.f32", F32).reshape(H, W, 3)
    score = gpu.sample_scores(dev(n), dev(mean), dev(m2), metric="relative", eps=1e-3).cpu().numpy()
    sel = [(int(a), int(b, 16), int(c), int(d)) for a, b, c, d in
           re.findall(r"select: rank (\d+) value 0x([0-9a-f]{8}) below (\d+) equal (\d+)", out.stdout)]
    px = W * H
    ranks = [px // 2, 0, px - 1, ref.nearest_rank(0.95, px), px // 2]
    want = ref.select_ref(score, ranks)
    assert sel == list(zip(want["rank"], want["value_bits"], want["n_below"], want["n_equal"]))
    assert len(set(want["value_bits"])) >= 3
    m = re.search(r"classes: px (\d+) live (\d+) saturated (\d+)", out.stdout)
    assert [int(g) for g in m.groups()] == [px, want["n_live"], want["n_saturated"]]
    above = [(int(b, 16), int(c)) for b, c in re.findall(r"above: threshold 0x([0-9a-f]{8}) count (\d+)", out.stdout)]
    th = from_bits([b for b, _ in above])
    assert [b for b, _ in above] == [0, want["value_bits"][0], 0x7F800000] and [c for _, c in above] == ref.count_above_ref(score, th)


def run_sim(build, stem, *extra):
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "64", "--height", "48", "--spp", "4", "--iterations", "3", "--threads", "4",
                          "--adaptive-pixels", "--stem", stem] + list(extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def dumps(stem):
    return {os.path.basename(p)[len(os.path.basename(stem)):]: open(p, "rb").read() for p in sorted(glob.glob(stem + "-*.pfm"))}


def test_render_loop_stops_at_a_quantile(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels --stop-at 0.95:T on 64 x 48, three iterations.  T = 0: never met, every iteration runs, no
    line -- and every dump equals, byte for byte, the run without the flag.  T = 1e30: met after the first iteration, whose 4 samples
    per pixel can be judged; one line, with the quantile of the dumped statistics; the dumps of that iteration are the unstopped
    run's."""
    from statmc_amd import build, pfm
    build.build_tools()
    plain, never, at_once = (str(tmp_path / s) for s in ("plain", "never", "at_once"))
    out_plain = run_sim(build, plain)
    out_never = run_sim(build, never, "--stop-at", "0.95:0")
    out_once = run_sim(build, at_once, "--stop-at", "0.95:1e30")
    steady = lambda text: [l for l in text.splitlines() if "[ns]" not in l]
    assert "Converged" not in out_plain and "Converged" not in out_never and steady(out_plain) == steady(out_never)
    assert len(re.findall(r"^Iteration: ", out_never, re.M)) == 3
    d_plain, d_never, d_once = dumps(plain), dumps(never), dumps(at_once)
    assert len(d_plain) > 10 and d_plain == d_never
    assert len(re.findall(r"^Iteration: ", out_once, re.M)) == 1 and "Planned" not in out_once
    lines = re.findall(r"^Converged: iteration (\d+), quantile (\S+) of the relative score = (\S+)$", out_once, re.M)
    assert len(lines) == 1 and lines[0][:2] == ("1", "0.95")
    assert d_once and all(k.startswith("-4-") and d_plain[k] == v for k, v in d_once.items())
    assert sorted(d_once) == sorted(k for k in d_plain if k.startswith("-4-"))
    rd = lambda what: np.asarray(pfm.read_pfm("%s-4-t0-b0-%s.pfm" % (at_once, what)))
    score = plan_ref.scores_ref(rd("n").astype(np.int32), rd("film-mean"), rd("film-m2"), plan_ref.RELATIVE, 1e-3)
    want = ref.select_ref(score, [ref.nearest_rank(0.95, 64 * 48)])
    assert np.array([lines[0][2]], np.float64).astype(F32).view(np.uint32)[0] == want["value_bits"][0] and 0 < float(lines[0][2]) <= 1e30
    # the flag alone, and a malformed one
    for bad in (["--stop-at", "0.95:1"], ["--adaptive-pixels", "--stop-at", "0.95"], ["--adaptive-pixels", "--stop-at", "1.5:1"]):
        r = subprocess.run([build.RENDER_SIM_BIN, "--width", "16", "--height", "16"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--stop-at" in r.stderr
