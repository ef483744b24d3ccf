"""statmc_score_sum on the device against the restatement in Python integers (tests/score_sum_reference.py, whose own cases
tests/test_score_sum_cpu.py checks): every field of the result bit for bit -- the doubles as uint64, the counts as integers -- no
tolerance anywhere; every class and exponent, constant images (every lane on one limb), several workgroups, unaligned images, a
workspace full of garbage, a shuffled image, guard bands, a library stream behind a gate and an event, FilmStats.score_mean and the
render loop's --stop-mean."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import score_sum_reference as ref
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
# one pixel; one partial quad and another; not a multiple of the quad or the wave; more than one workgroup's step, odd; 65 workgroups
FILMS = [(1, 1), (7, 1), (67, 5), (257, 33), (1024, 65)]
IMAGES = ["random_bits", "constant_normal", "constant_smallest_subnormal", "constant_largest_finite", "two_bands"]
CONSTANTS = {"constant_normal": 0x3F400000, "constant_smallest_subnormal": 0x00000001, "constant_largest_finite": 0x7F7FFFFF}
SCORE_FILM = (64, 48)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def dev_offset(a):
    """the same values in an image that starts 4 bytes into its allocation: 4-byte but not 16-byte aligned"""
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
    if name == "random_bits":      # every class and exponent; the rare ones put in by hand where the film has room
        b = rng.integers(0, 2 ** 32, px, dtype=np.uint64).astype(np.uint32)
        special = [0x7FC00000, 0xFFC00001, 0x80000000, 0xBF800000, 0x00000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x00800000, 0x7F7FFFFF, 0]
        if px > 2 * len(special):
            b[rng.choice(px, len(special), replace=False)] = special
        return from_bits(b).reshape(H, W)
    if name in CONSTANTS:
        return from_bits(np.full((H, W), CONSTANTS[name], np.uint32))
    if name == "two_bands":        # a lane's run changes its limbs at every quad: 2^-20 .. 2^-5 in even quads, 2^12 .. 2^27 in odd ones
        at = np.arange(px) // 4 % 2
        e = np.where(at == 0, rng.integers(107, 123, px), rng.integers(139, 155, px)).astype(np.uint32)
        return from_bits((e << np.uint32(23)) | rng.integers(0, 1 << 23, px).astype(np.uint32)).reshape(H, W)
    raise KeyError(name)


def cap_sets(score):
    """+inf alone; four unsorted with a repeat; a value present in the image, alone and beside its neighbours; +0 and a negative cap;
    subnormal caps"""
    keys = np.sort(ref.keys_of(score))
    present = int(keys[keys.size // 2])
    up, down = min(present + 1, 0x7F800000), max(present - 1, 0)
    return [[INF], [F32(2.0), F32(1e-3), F32(2.0), F32(3e30)], [from_bits([present])[0]],
            [from_bits([up])[0], from_bits([present])[0], INF, from_bits([down])[0]], [F32(0.0), F32(-1.5)],
            [from_bits([0x00000123])[0], from_bits([0x00700000])[0], F32(1e-20)]]


_cases = {}


def case(film, name):
    """(score image, {caps as bits: the restatement's result}), computed once and left unchanged"""
    if (film, name) not in _cases:
        W, H = film
        score = image(name, W, H)
        score.setflags(write=False)
        want = {tuple(int(b) for b in np.asarray(c, F32).view(np.uint32)): ref.sum_ref(score, c) for c in cap_sets(score)}
        _cases[(film, name)] = (score, want)
    return _cases[(film, name)]


def run(gpu, d_score, caps, **kw):
    import torch
    res = gpu.score_sum(d_score, caps, **kw)
    if "stream" not in kw:
        torch.cuda.synchronize()
    return res


def whole_struct(gpu, t):
    """the 152 bytes as the device wrote them, as integers: the doubles as their bit patterns, the slots behind n_caps and the pad"""
    raw = t.cpu().numpy().tobytes()[:C.sizeof(gpu.SumResult)]
    r = gpu.SumResult.from_buffer_copy(raw)
    d = np.frombuffer(raw, np.uint64)
    return ([int(r.n_px), int(r.n_zero), int(r.n_finite), int(r.n_infinite), int(r.n_caps), int(r.pad)] + [int(v) for v in r.cap_bits]
            + [int(v) for v in r.n_clipped] + [int(v) for v in d[11:19]])


def whole_want(w):
    """the same list from a restated result: slots n_caps .. 3 are 0"""
    return ([w["n_px"], w["n_zero"], w["n_finite"], w["n_infinite"], w["n_caps"], 0] + list(w["cap_bits"]) + list(w["n_clipped"])
            + [ref.double_bits(x) for x in w["sum"]] + [ref.double_bits(x) for x in w["sum_sq"]])


@pytest.mark.parametrize("name", IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_sum_equals_the_restatement_bit_for_bit(gpu, film, name):
    import torch
    score, want = case(film, name)
    d_score = dev(score)
    for caps, w in want.items():
        c = from_bits(list(caps))
        t = run(gpu, d_score, c)
        raw = whole_struct(gpu, t)
        assert raw == whole_want(w), (caps, raw, whole_want(w))
        got = gpu.read_sum_result(t)
        assert ref.result_bits({**got, "cap_bits": got["cap_bits"] + [0] * (4 - len(caps)), "n_clipped": got["n_clipped"] + [0] * (4 - len(caps)),
                                "sum": got["sum"] + [0.0] * (4 - len(caps)), "sum_sq": got["sum_sq"] + [0.0] * (4 - len(caps))}) == ref.result_bits(w)
        assert got["n_zero"] + got["n_finite"] + got["n_infinite"] == got["n_px"] == score.size
        k = len(caps)
        assert raw[5] == 0 and raw[6 + k:10] == [0] * (4 - k) and raw[10 + k:14] == [0] * (4 - k)      # slots n_caps .. 3 are written as 0
        assert raw[14 + k:18] == [0] * (4 - k) and raw[18 + k:22] == [0] * (4 - k)
        above = gpu.score_count_above(d_score, c)      # n_clipped is statmc_score_count_above's
        torch.cuda.synchronize()
        assert [int(v) for v in above.cpu().numpy()] == got["n_clipped"]
    px = score.size
    if name in CONSTANTS:      # every lane on the same limbs: n times the value, exactly
        w = want[(0x7F800000,)]
        u = ref.units_of(CONSTANTS[name])
        assert w["n_finite"] == px and w["sum"][0] == ref.round_to_double(px * u, 149) and w["sum_sq"][0] == ref.round_to_double(px * u * u, 298)
    zero = [w for caps, w in want.items() if caps[0] == 0][0]
    assert zero["sum"][:2] == [0.0, 0.0] and zero["sum_sq"][:2] == [0.0, 0.0] and zero["n_clipped"][0] == zero["n_finite"] + zero["n_infinite"]
    if name == "random_bits" and px > 1000:
        w = want[(0x7F800000,)]
        assert w["n_zero"] > px // 3 and w["n_infinite"] >= 1 and w["n_finite"] > px // 3 and w["sum"][0] > 1e30


@pytest.mark.parametrize("name", ["random_bits", "constant_normal", "two_bands"])
@pytest.mark.parametrize("film", [(7, 1), (67, 5), (1024, 65)], ids=lambda f: "%dx%d" % f)
def test_unaligned_images_take_the_element_path_to_the_same_bits(gpu, film, name):
    score, want = case(film, name)
    d_score = dev_offset(score)
    for caps, w in want.items():
        assert whole_struct(gpu, run(gpu, d_score, from_bits(list(caps)))) == whole_want(w), caps


@pytest.mark.parametrize("name", ["random_bits", "two_bands"])
@pytest.mark.parametrize("film", [(67, 5), (1024, 65)], ids=lambda f: "%dx%d" % f)
def test_a_shuffled_image_two_runs_and_a_workspace_full_of_garbage_give_the_same_bits(gpu, film, name):
    import torch
    score, want = case(film, name)
    caps = [c for c in want if len(c) == 4][0]
    c = from_bits(list(caps))
    d_score = dev(score)
    first = whole_struct(gpu, run(gpu, d_score, c))
    assert first == whole_want(want[caps]) and whole_struct(gpu, run(gpu, d_score, c)) == first
    shuffled = np.random.default_rng(3).permutation(score.reshape(-1)).reshape(score.shape)
    assert not np.array_equal(shuffled.view(np.uint32), score.view(np.uint32))
    assert whole_struct(gpu, run(gpu, dev(shuffled), c)) == first      # integer additions commute: no order reaches a bit
    ws = torch.full((gpu.score_sum_workspace(),), 0xFF, dtype=torch.uint8, device="cuda:0")
    result = torch.full((19,), -1, dtype=torch.int64, device="cuda:0")
    t = run(gpu, d_score, c, workspace=ws, result=result)
    assert t.data_ptr() == result.data_ptr() and whole_struct(gpu, t) == first


def test_only_the_result_and_the_workspace_are_written(gpu):
    """guard bands of 0xA5 bytes on both sides of the workspace and of the result, and the score image's bytes before and after"""
    import torch
    score, want = case((257, 33), "random_bits")
    caps = [c for c in want if len(c) == 4][0]
    need, band = gpu.score_sum_workspace(), 256
    ws = torch.full((band + need + band,), 0xA5, dtype=torch.uint8, device="cuda:0")
    res = torch.full((32 + 19 + 32,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    d_score = dev(score)
    before = d_score.view(torch.int32).cpu().numpy().copy()
    t = run(gpu, d_score, from_bits(list(caps)), workspace=ws[band:band + need], result=res[32:32 + 19])
    assert whole_struct(gpu, t) == whole_want(want[caps])
    host = ws.cpu().numpy()
    assert np.all(host[:band] == 0xA5) and np.all(host[band + need:] == 0xA5)
    host = res.cpu().numpy()
    assert np.all(host[:32] == 0x5A5A5A5A5A5A5A5A) and np.all(host[32 + 19:] == 0x5A5A5A5A5A5A5A5A)
    assert np.array_equal(d_score.view(torch.int32).cpu().numpy(), before) and np.array_equal(before.view(np.uint32), score.view(np.uint32))


def error_score_film(gpu):
    """64 x 48, 2 to 9 samples per pixel, every 11th pixel 0 or 1 samples: (FilmStats, its relative standard-error image on the host)"""
    import torch
    from statmc_amd.film import FilmStats
    W, H = SCORE_FILM
    names = ("radiance", "normal", "albedo")
    _, smp, _ = make_case(W, H, 9)
    rng = np.random.default_rng(17)
    counts = rng.integers(2, 10, (H, W)).astype(np.int32)
    counts.reshape(-1)[::11] = rng.integers(0, 2, counts.reshape(-1)[::11].size)
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names}, counts=dev(counts))
    rad = film.state["radiance"]
    score = gpu.error_scores(rad["n"], rad["film_mean"], rad["film_m2"], metric="relative", eps=1e-3, table="stderr")
    torch.cuda.synchronize()
    return film, score, counts


def test_an_image_of_error_scores_and_film_stats_score_mean(gpu):
    film, d_score, counts = error_score_film(gpu)
    score = d_score.cpu().numpy()
    unjudged = int((counts < 2).sum())
    assert unjudged > 100 and int(np.isinf(score).sum()) == unjudged
    for caps in ([INF], [F32(0.05), INF, F32(1.0), F32(0.05)], [float(np.median(score))]):
        w = ref.sum_ref(score, caps)
        assert whole_struct(gpu, run(gpu, d_score, caps)) == whole_want(w), caps
        got = film.score_mean(caps=caps, metric="relative", eps=1e-3, error="stderr")
        assert [(ref.double_bits(m), ref.double_bits(r)) for m, r in zip(got["mean"], got["rms"])] == \
               [(ref.double_bits(m), ref.double_bits(r)) for m, r in ref.means(w)], caps
        assert (got["n_px"], got["n_zero"], got["n_finite"], got["n_infinite"], got["n_clipped"]) == \
               (w["n_px"], w["n_zero"], w["n_finite"], w["n_infinite"], w["n_clipped"][:len(caps)])
    got = film.score_mean()      # no cap: over the judged pixels alone
    assert got["n_infinite"] == unjudged and 0 < got["mean"][0] <= got["rms"][0] < 10
    judged = score[np.isfinite(score)].astype(np.float64)
    assert abs(got["mean"][0] - judged.mean()) <= 1e-12 * judged.mean()      # (the exact sum against a float64 one: close, not equal)
    # the window in front: the pipeline of score_quantiles
    wide = gpu.score_window(d_score, 2, "max").cpu().numpy()
    got = film.score_mean(caps=[1.0], dilate=2)
    assert (ref.double_bits(got["mean"][0]), ref.double_bits(got["rms"][0])) == tuple(ref.double_bits(x) for x in ref.means(ref.sum_ref(wide, [1.0]))[0])
    with pytest.raises(gpu.StatmcError, match="n_caps"):
        film.score_mean(caps=[])


def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(8, 8, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="n_caps"):
        gpu.score_sum(score, [])
    with pytest.raises(gpu.StatmcError, match="n_caps"):
        gpu.score_sum(score, [1.0] * 5)
    with pytest.raises(gpu.StatmcError, match=r"caps\[1\] is NaN"):
        gpu.score_sum(score, [1.0, float("nan")])
    with pytest.raises(gpu.StatmcError, match="workspace_bytes"):
        gpu.score_sum(score, [1.0], workspace=torch.empty(64, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(gpu.StatmcError, match="result overlaps score"):
        gpu.score_sum(score, [1.0], result=score.view(torch.int64))


# ---------------------------------------------------------------- the stream contract
def test_the_entry_runs_on_its_stream_and_an_event_makes_the_result_visible(gpu):
    """The gate of tests/test_stream_contract_gpu.py: on a non-blocking library stream, the score image, a workspace and a result full
    of poison are overwritten behind a closed gate, then the entry, then the read-back, all on that stream -- anything the entry put
    on another stream would see the poison.  Then an event recorded behind a second call on the side stream, which the null stream
    waits for: what the null stream reads is the result."""
    import torch
    from test_stream_contract_gpu import Case, assert_same_bits, run_gated, run_on_null_stream, stream_apart_from_the_null_stream
    api, lib = gpu, gpu.load()
    score, want = case((1024, 65), "random_bits")
    caps = [c for c in want if len(c) == 4][0]
    assert torch.cuda.current_stream().cuda_stream == 0
    side, gate = stream_apart_from_the_null_stream(api)
    event = C.c_void_p()
    api.check(lib.statmc_event_create(C.byref(event)))
    try:
        c = Case("score_sum-1024x65")
        other, _ = case((1024, 65), "two_bands")
        d_score = c.live(np.array(score), b=np.array(other))
        ws = c.live(np.zeros(api.score_sum_workspace(), np.uint8))
        res = c.live(np.zeros(19, np.int64), b=np.full(19, -1, np.int64), out="result")
        c.call = lambda stream: api.score_sum(d_score, from_bits(list(caps)), workspace=ws, result=res, stream=stream)
        on_null = run_on_null_stream(c)
        gated = run_gated(api, c, side, gate)
        assert_same_bits(c, gated, on_null, "gated on the side stream against the null-stream run")
        assert whole_struct(api, torch.from_numpy(c.res("result"))) == whole_want(want[caps])
        # the event
        res.fill_(-1)
        torch.cuda.synchronize()
        c.call(side.handle)
        api.check(lib.statmc_event_record(event, side.handle))
        api.check(lib.statmc_stream_wait_event(None, event))
        seen = res.clone()      # on the null stream, behind the event
        torch.cuda.current_stream().synchronize()
        assert whole_struct(api, seen) == whole_want(want[caps])
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_event_destroy(event))
        side.destroy()


# ---------------------------------------------------------------- the render loop
def run_sim(build, stem, *extra):
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "64", "--height", "48", "--spp", "4", "--iterations", "3", "--threads", "4",
                          "--adaptive-pixels", "--stop-metric", "stderr", "--stem", stem] + list(extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_render_loop_stops_at_a_mean(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels --stop-mean on 64 x 48, three iterations.  A target of 0 is never met: every iteration
    runs and prints its line.  A target of 1e30 is met after the first iteration; the printed mean / RMS equals, to the printed
    digits, the restatement on the score of the statistics that iteration dumped."""
    from statmc_amd import build, pfm
    import error_reference as err_ref
    import plan_reference as plan_ref
    build.build_tools()
    for rule, cap in (("mean", None), ("rms", None), ("mean", 0.25), ("rms", 0.25)):
        stem = str(tmp_path / ("%s_%s" % (rule, cap)))
        arg = "%s:1e30" % rule + (":%g" % cap if cap is not None else "")
        out = run_sim(build, stem, "--stop-mean", arg)
        assert len(re.findall(r"^Iteration: ", out, re.M)) == 1 and "Planned" not in out
        lines = re.findall(r"^Mean rule: iteration (\d+), (mean|rms) of the relative standard error under (\S+) = (\S+) over (\d+) pixels, target (\S+): (met|open)$", out, re.M)
        assert len(lines) == 1 and lines[0][:2] == ("1", rule) and lines[0][6] == "met", out
        rd = lambda what: np.asarray(pfm.read_pfm("%s-4-t0-b0-%s.pfm" % (stem, what)))
        score = err_ref.error_scores_ref(rd("n").astype(np.int32), rd("film-mean"), rd("film-m2"), plan_ref.RELATIVE, 1e-3, None)
        w = ref.sum_ref(score, [cap if cap is not None else INF])
        mean, rms = ref.means(w)[0]
        assert lines[0][3] == "%.9g" % (mean if rule == "mean" else rms), (lines[0], mean, rms)
        assert int(lines[0][4]) == w["n_px"] - (w["n_infinite"] if cap is None else 0) and float(lines[0][2]) == (cap if cap is not None else INF)
    never = run_sim(build, str(tmp_path / "never"), "--stop-mean", "mean:0")
    assert len(re.findall(r"^Iteration: ", never, re.M)) == 3 and len(re.findall(r"^Mean rule: .*: open$", never, re.M)) == 3 and ": met" not in never
    both = run_sim(build, str(tmp_path / "both"), "--stop-mean", "mean:1e30", "--stop-at", "0.95:0")      # both must hold
    assert len(re.findall(r"^Iteration: ", both, re.M)) == 3 and "Converged" not in both
    for bad in (["--stop-mean", "mean:1"], ["--adaptive-pixels", "--stop-mean", "mean"], ["--adaptive-pixels", "--stop-mean", "median:1"],
                ["--adaptive-pixels", "--stop-mean", "rms:-1"], ["--adaptive-pixels", "--preview", "2", "--stop-mean", "mean:1"]):
        r = subprocess.run([build.RENDER_SIM_BIN, "--width", "16", "--height", "16"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--stop-mean" in r.stderr, (bad, r.stderr)
