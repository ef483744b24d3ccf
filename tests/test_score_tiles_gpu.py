"""statmc_score_tiles on the device against the restatement in Python integers and Fractions (tests/score_tiles_reference.py, whose
own cases tests/test_score_tiles_cpu.py checks): every plane bit for bit -- the doubles as uint64, the floats as uint32, the counts as
integers -- no tolerance anywhere.  Every tile size on films with partial tiles, one pixel, more than one workgroup; every class and
exponent, constant images, ties of the double and of the float rounding; NULL planes, unaligned images, planes full of garbage, pixels
shuffled within their tiles, guard words; statmc_score_sum, statmc_score_select, statmc_score_count_above and statmc_compact_offsets
on the same data; a library stream behind a gate and an event; FilmStats.score_tiles and the render loop's --stop-tiles."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import score_sum_reference as sum_ref
import score_tiles_reference as ref
from conftest import make_case

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
# one pixel; the float-tie film; a partial tile of every size; exactly one 8-tile; one pixel over it; rows shorter than a quad apart;
# exactly one 64-tile; one pixel over it in x, a partial one in y; more rows than columns, three tiles of 64 down; five tiles of 64 across
FILMS = [(1, 1), (2, 1), (7, 3), (8, 8), (9, 9), (17, 5), (64, 64), (65, 33), (67, 130), (257, 70)]
IMAGES = ["random_bits", "constant_normal", "constant_subnormal", "all_infinite", "all_zero", "two_bands", "extremes", "double_tie_1", "double_tie_3"]
CONSTANTS = {"constant_normal": 0x3F400000, "constant_subnormal": 0x00000301, "all_infinite": 0x7F800000, "all_zero": 0}
SUBSET = ("mean", "max", "n_clipped")
NO_CAP, ZERO_CAP, NEGATIVE_CAP = 0x7F800000, 0x00000000, 0xBFC00000      # the caps every case has, as float bits: +inf, +0, -1.5


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
    if name == "extremes":         # 2^-149 and the largest finite float in every tile of 8, ones between
        b = np.full((H, W), 0x3F800000, np.uint32)
        b[::8, ::8] = 0x00000001
        b[(H > 1)::8, (W > 1)::8] = 0x7F7FFFFF
        return from_bits(b)
    if name.startswith("double_tie_"):      # 2^-96 and one or three pixels of 2^-149 in the first tile: half a double's unit, and three halves
        b = np.zeros((H, W), np.uint32)
        first = [(y, x) for y in range(min(H, 8)) for x in range(min(W, 8))][:1 + int(name[-1])]
        for i, (y, x) in enumerate(first):
            b[y, x] = (127 - 96) << 23 if i == 0 else 1
        return from_bits(b)
    raise KeyError(name)


def caps_of(score):
    """+inf: no cap; a value present in the image (the median of its finite non-zero keys; 1 where it has none); +0; a negative cap,
    which is +0's key"""
    keys = np.sort(sum_ref.keys_of(score))
    live = keys[(keys > 0) & (keys < sum_ref.INF_KEY)]
    return [INF, from_bits([int(live[live.size // 2]) if live.size else 0x3F800000])[0], F32(0.0), F32(-1.5)]


def mid_cap(want, tile):
    """the bits of the case's cap that is neither +inf nor +0's key"""
    return [c for (t, c) in want if t == tile and c not in (NO_CAP, ZERO_CAP, NEGATIVE_CAP)][0]


_cases = {}


def case(film, name):
    """(score image, {(tile, cap bits): the restated planes}), computed once and left unchanged"""
    if (film, name) not in _cases:
        W, H = film
        score = image(name, W, H)
        score.setflags(write=False)
        want = {}
        for tile in ref.TILES:
            for cap in caps_of(score):
                w = ref.tiles_ref(score, tile, cap)
                for a in w.values():
                    a.setflags(write=False)
                want[(tile, int(np.asarray([cap], F32).view(np.uint32)[0]))] = w
        _cases[(film, name)] = (score, want)
    return _cases[(film, name)]


def run(gpu, d_score, tile, cap_bits, planes=ref.PLANES, **kw):
    import torch
    res = gpu.score_tiles(d_score, tile, from_bits([cap_bits])[0], planes=planes, **kw)
    if "stream" not in kw:
        torch.cuda.synchronize()
    return gpu.read_tile_scores(res)


def assert_planes(got, want, what, planes=ref.PLANES):
    assert sorted(got) == sorted(planes), what
    differ = ref.same_bits(got, want, planes)
    if differ:
        p = differ[0]
        g, w = ref.plane_bits(got[p]), ref.plane_bits(want[p])
        at = np.argwhere(g != w)[0] if g.shape == w.shape else None
        detail = "" if at is None else " first at tile %s: %x, restated %x" % (tuple(at), int(g[tuple(at)]), int(w[tuple(at)]))
        raise AssertionError("%s: planes %s differ;%s" % (what, differ, detail))


# ---------------------------------------------------------------- 1. every plane, every tile size, bit for bit
@pytest.mark.parametrize("name", IMAGES)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_tiles_equal_the_restatement_bit_for_bit(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    W, H = film
    for (tile, cap), w in want.items():
        got = run(gpu, d_score, tile, cap)
        assert_planes(got, w, (film, name, tile, hex(cap)))
        assert got["sum"].shape == (-(-H // tile), -(-W // tile)) == gpu.tile_grid(H, W, tile)
        assert int(got["n_px"].sum()) == W * H and got["n_px"].max() <= tile * tile
        assert not np.isnan(got["mean"]).any() and not np.signbit(got["mean"]).any() and not np.isnan(got["max"]).any()
    tile, cap = ref.TILES[(W + H) % 4], NO_CAP
    assert_planes(run(gpu, d_score, tile, cap, planes=SUBSET), want[(tile, cap)], (film, name, "three planes"), SUBSET)      # the others NULL
    for p in ref.PLANES:
        assert_planes(run(gpu, d_score, tile, cap, planes=(p,)), want[(tile, cap)], (film, name, "one plane", p), (p,))
    # what the images are for
    no_cap = want[(8, 0x7F800000)]
    if name == "constant_normal":
        u = sum_ref.units_of(CONSTANTS[name])
        assert np.all(no_cap["mean"].view(np.uint32) == CONSTANTS[name]) and no_cap["sum"][0, 0] == sum_ref.round_to_double(int(no_cap["n_px"][0, 0]) * u, 149)
    if name == "all_infinite":
        assert np.all(no_cap["mean"] == 0) and np.all(no_cap["sum"] == 0) and np.all(no_cap["n_infinite"] == no_cap["n_px"]) and np.all(np.isinf(no_cap["max"]))
    if name == "extremes" and W > 1 and H > 1:
        assert no_cap["max"].view(np.uint32)[0, 0] == 0x7F7FFFFF and no_cap["sum"][0, 0] > 3e38 and np.isfinite(no_cap["mean"]).all()
    if name.startswith("double_tie_") and min(W, 8) * min(H, 8) >= 4:      # the restatement itself goes to even both ways
        tie = want[(64, 0x7F800000)]["sum"][0, 0]
        assert tie == (2.0 ** -96 if name[-1] == "1" else 2.0 ** -96 + 2.0 ** -147)
    zero = want[(16, 0)]
    assert np.all(zero["sum"] == 0) and np.all(zero["mean"] == 0) and np.array_equal(zero["n_clipped"], zero["n_px"] - zero["n_zero"])
    assert_planes(want[(32, NEGATIVE_CAP)], want[(32, ZERO_CAP)], "a negative cap is +0's key")


def test_a_float_mean_tie_goes_to_even_in_both_parities(gpu):
    """2 x 1: a and the next float.  Their mean lies half way: it rounds to the one with the even significand."""
    for a, even in ((0x3F800000, 0x3F800000), (0x3F800001, 0x3F800002), (0x00000002, 0x00000002), (0x00000003, 0x00000004),
                    (0x007FFFFF, 0x00800000), (0x7F7FFFFE, 0x7F7FFFFE)):
        score = from_bits([[a, a + 1]])
        for tile in ref.TILES:
            w = ref.tiles_ref(score, tile, INF)
            assert int(w["mean"].view(np.uint32)[0, 0]) == even, hex(a)
            for d in (dev(score), dev_offset(score)):
                assert_planes(run(gpu, d, tile, 0x7F800000), w, (hex(a), tile))


# ---------------------------------------------------------------- 2. the element path
@pytest.mark.parametrize("name", ["random_bits", "two_bands", "extremes"])
@pytest.mark.parametrize("film", [(7, 3), (9, 9), (65, 33), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_unaligned_images_take_the_element_path_to_the_same_bits(gpu, film, name):
    score, want = case(film, name)
    d_score = dev_offset(score)
    for (tile, cap), w in want.items():
        assert_planes(run(gpu, d_score, tile, cap), w, (film, name, tile, hex(cap)))


# ---------------------------------------------------------------- 3. no order reaches a bit
def shuffled_within_tiles(score, tile, seed=3):
    out = np.array(score)
    rng = np.random.default_rng(seed)
    H, W = out.shape
    for y in range(0, H, tile):
        for x in range(0, W, tile):
            block = out[y:y + tile, x:x + tile]
            out[y:y + tile, x:x + tile] = rng.permutation(block.reshape(-1)).reshape(block.shape)
    return out


@pytest.mark.parametrize("name", ["random_bits", "two_bands"])
@pytest.mark.parametrize("film", [(67, 130), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_two_runs_a_shuffle_within_tiles_and_planes_full_of_garbage_give_the_same_bits(gpu, film, name):
    import torch
    score, want = case(film, name)
    d_score = dev(score)
    W, H = film
    for (tile, cap), w in want.items():
        if cap in (ZERO_CAP, NEGATIVE_CAP):
            continue
        assert_planes(run(gpu, d_score, tile, cap), w, "first")
        assert_planes(run(gpu, d_score, tile, cap), w, "second")
        mixed = shuffled_within_tiles(score, tile)
        assert not np.array_equal(mixed.view(np.uint32), score.view(np.uint32))
        assert_planes(run(gpu, dev(mixed), tile, cap), w, "shuffled within tiles")
        shape = gpu.tile_grid(H, W, tile)
        out = {p: torch.full(shape, -1 if ref.DTYPES[p] == np.int32 else float("nan"), dtype=getattr(torch, np.dtype(ref.DTYPES[p]).name), device="cuda:0")
               for p in ref.PLANES}
        got = run(gpu, d_score, tile, cap, out=out)
        assert_planes(got, w, "planes full of garbage")


# ---------------------------------------------------------------- 4. - 6. the family's other entries on the same pixels
@pytest.mark.parametrize("name", ["random_bits", "two_bands", "extremes", "all_infinite"])
@pytest.mark.parametrize("film", [f for f in FILMS if f[0] <= 64 and f[1] <= 64], ids=lambda f: "%dx%d" % f)
def test_one_tile_over_the_film_is_score_sum_and_score_select(gpu, film, name):
    import torch
    score, want = case(film, name)
    d_score = dev(score)
    for (tile, cap) in want:
        if tile != 64:
            continue
        got = run(gpu, d_score, 64, cap)
        assert got["sum"].shape == (1, 1)
        whole = gpu.read_sum_result(gpu.score_sum(d_score, [from_bits([cap])[0]]))
        assert (sum_ref.double_bits(got["sum"][0, 0]), sum_ref.double_bits(got["sum_sq"][0, 0])) == \
               (sum_ref.double_bits(whole["sum"][0]), sum_ref.double_bits(whole["sum_sq"][0])), (film, name, hex(cap))
        assert (int(got["n_clipped"][0, 0]), int(got["n_zero"][0, 0]), int(got["n_infinite"][0, 0]), int(got["n_px"][0, 0])) == \
               (whole["n_clipped"][0], whole["n_zero"], whole["n_infinite"], whole["n_px"])
        top = gpu.read_select_result(gpu.score_select(d_score, [score.size - 1]))
        torch.cuda.synchronize()
        assert int(got["max"].view(np.uint32)[0, 0]) == top["value_bits"][0]


@pytest.mark.parametrize("name", ["random_bits", "two_bands"])
@pytest.mark.parametrize("film", [(64, 64), (67, 130), (257, 70)], ids=lambda f: "%dx%d" % f)
def test_a_tile_of_64_is_composed_of_its_sixteen_tiles_of_16(gpu, film, name):
    score, want = case(film, name)
    d_score = dev(score)
    cap = mid_cap(want, 64)
    big, small = run(gpu, d_score, 64, cap), run(gpu, d_score, 16, cap)
    ty, tx = big["n_px"].shape
    for j in range(ty):
        for i in range(tx):
            block = {p: small[p][4 * j:4 * j + 4, 4 * i:4 * i + 4] for p in small}
            for p in ("n_px", "n_zero", "n_infinite", "n_clipped"):
                assert int(block[p].sum()) == int(big[p][j, i]), (p, j, i)
            assert int(block["max"].view(np.uint32).max()) == int(big["max"].view(np.uint32)[j, i])


# ---------------------------------------------------------------- 7. the planes are score and count images of the tile grid
def test_the_planes_go_through_count_above_select_and_compact_offsets(gpu):
    import torch
    score, want = case((257, 70), "random_bits")
    d_score = dev(score)
    for tile in ref.TILES:
        cap = mid_cap(want, tile)
        w = want[(tile, cap)]
        res = gpu.score_tiles(d_score, tile, from_bits([cap])[0])
        ty, tx = w["mean"].shape
        for plane in ("mean", "max"):
            keys = np.sort(w[plane].view(np.uint32).reshape(-1))
            thresholds = [from_bits([int(keys[keys.size // 2])])[0], F32(0.0), from_bits([int(keys[-1])])[0]]
            above = gpu.score_count_above(res[plane], thresholds).cpu().numpy()
            assert [int(v) for v in above] == [int((keys > ref.key_of(t)).sum()) for t in thresholds], (tile, plane)
            ranks = [0, keys.size // 2, keys.size - 1]
            sel = gpu.read_select_result(gpu.score_select(res[plane], ranks))
            assert sel["value_bits"] == [int(keys[r]) for r in ranks], (tile, plane)
        offsets, owners = gpu.compact_offsets(res["n_clipped"], cap=1, owners_capacity=ty * tx)      # the open tiles, in raster order
        torch.cuda.synchronize()
        open_tiles = np.flatnonzero(w["n_clipped"].reshape(-1) > 0)
        assert int(offsets[-1].item()) == open_tiles.size and 0 < open_tiles.size
        assert np.array_equal(owners.cpu().numpy()[:open_tiles.size], open_tiles) and np.all(owners.cpu().numpy()[open_tiles.size:] == -1)


# ---------------------------------------------------------------- 8. only the planes are written
def test_only_the_planes_are_written(gpu):
    """each plane lies between guard words in a buffer of its own; the score image's bytes before and after"""
    import torch
    score, want = case((257, 70), "random_bits")
    d_score = dev(score)
    before = d_score.view(torch.int32).cpu().numpy().copy()
    guard = 64
    for tile in ref.TILES:
        cap = 0x7F800000
        ty, tx = gpu.tile_grid(70, 257, tile)
        bufs, out = {}, {}
        for p in ref.PLANES:
            dt = getattr(torch, np.dtype(ref.DTYPES[p]).name)
            bufs[p] = torch.full((guard + ty * tx + guard,), 7, dtype=dt, device="cuda:0")
            out[p] = bufs[p][guard:guard + ty * tx].view(ty, tx)
        assert_planes(run(gpu, d_score, tile, cap, out=out), want[(tile, cap)], tile)
        for p in ref.PLANES:
            host = bufs[p].cpu().numpy()
            assert np.all(host[:guard] == 7) and np.all(host[guard + ty * tx:] == 7), (tile, p)
    assert np.array_equal(d_score.view(torch.int32).cpu().numpy(), before) and np.array_equal(before.view(np.uint32), score.view(np.uint32))


# ---------------------------------------------------------------- 9. refusals, with a device
def test_invalid_calls_are_refused_with_a_device_too(gpu):
    import torch
    score = torch.ones(16, 16, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="tile = 12"):
        gpu.score_tiles(score, 12)
    with pytest.raises(gpu.StatmcError, match="tile = 128"):
        gpu.score_tiles(score, 128)
    with pytest.raises(gpu.StatmcError, match="cap is NaN"):
        gpu.score_tiles(score, 8, float("nan"))
    with pytest.raises(gpu.StatmcError, match="every plane"):
        gpu.score_tiles(score, 8, planes=())
    with pytest.raises(gpu.StatmcError, match="out->mean overlaps score"):
        gpu.score_tiles(score, 8, planes=("mean",), out={"mean": score.view(-1)[:4].view(2, 2)})
    shared = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    with pytest.raises(gpu.StatmcError, match="out->n_zero overlaps out->n_px"):
        gpu.score_tiles(score, 8, planes=("n_px", "n_zero"), out={"n_px": shared[:4].view(2, 2), "n_zero": shared[2:6].view(2, 2)})
    lib = gpu.load()
    ptrs = gpu.TileScores()
    ptrs.sum = shared.data_ptr() + 4
    assert lib.statmc_score_tiles(16, 16, score.data_ptr(), 8, C.c_float(1.0), C.byref(ptrs), None) == gpu.ERR_INVALID
    assert "out->sum is not 8-byte aligned" in lib.statmc_last_error().decode()
    assert lib.statmc_score_tiles(16, 16, score.data_ptr(), 8, C.c_float(1.0), None, None) == gpu.ERR_INVALID and b"null out" in lib.statmc_last_error()


# ---------------------------------------------------------------- 10. the stream contract
def test_the_entry_runs_on_its_stream_and_an_event_makes_the_planes_visible(gpu):
    """The gate of tests/test_stream_contract_gpu.py: on a non-blocking library stream, the score image and planes full of poison
    are overwritten behind a closed gate, then the entry, then the read-back, all on that stream -- anything the entry put on another
    stream would see the poison.  Then an event recorded behind a second call on the side stream, which the null stream waits for:
    what the null stream reads is the planes."""
    import torch
    from test_stream_contract_gpu import Case, assert_same_bits, run_gated, run_on_null_stream, stream_apart_from_the_null_stream
    api, lib = gpu, gpu.load()
    film = (257, 70)
    score, want = case(film, "random_bits")
    other, _ = case(film, "two_bands")
    tile, cap = 16, mid_cap(want, 16)
    w = want[(tile, cap)]
    assert torch.cuda.current_stream().cuda_stream == 0
    side, gate = stream_apart_from_the_null_stream(api)
    event = C.c_void_p()
    api.check(lib.statmc_event_create(C.byref(event)))
    try:
        c = Case("score_tiles-257x70")
        d_score = c.live(np.array(score), b=np.array(other))
        out = {p: c.live(np.zeros(w[p].shape, ref.DTYPES[p]), b=np.full(w[p].shape, 5, ref.DTYPES[p]), out=p) for p in ref.PLANES}
        c.call = lambda stream: api.score_tiles(d_score, tile, from_bits([cap])[0], out=out, stream=stream)
        on_null = run_on_null_stream(c)
        gated = run_gated(api, c, side, gate)
        assert_same_bits(c, gated, on_null, "gated on the side stream against the null-stream run")
        assert_planes({p: c.res(p) for p in ref.PLANES}, w, "gated")
        # the event
        for t in out.values():
            t.fill_(5)
        torch.cuda.synchronize()
        c.call(side.handle)
        api.check(lib.statmc_event_record(event, side.handle))
        api.check(lib.statmc_stream_wait_event(None, event))
        seen = {p: t.clone() for p, t in out.items()}      # on the null stream, behind the event
        torch.cuda.current_stream().synchronize()
        assert_planes({p: t.cpu().numpy() for p, t in seen.items()}, w, "behind the event")
    finally:
        torch.cuda.synchronize()
        api.check(lib.statmc_event_destroy(event))
        side.destroy()


# ---------------------------------------------------------------- 11. FilmStats
def test_film_stats_score_tiles_on_an_accumulated_film(gpu):
    import torch
    from statmc_amd.film import FilmStats
    W, H = 64, 48
    names = ("radiance", "normal", "albedo")
    _, smp, _ = make_case(W, H, 9)
    rng = np.random.default_rng(17)
    counts = rng.integers(2, 10, (H, W)).astype(np.int32)
    counts.reshape(-1)[::11] = rng.integers(0, 2, counts.reshape(-1)[::11].size)
    film = FilmStats(W, H, torch.device("cuda:0"), types=names)
    film.accumulate({t: dev(smp[t]) for t in names}, counts=dev(counts))
    rad = film.state["radiance"]
    score = gpu.error_scores(rad["n"], rad["film_mean"], rad["film_m2"], metric="relative", eps=1e-3, table="stderr").cpu().numpy()
    assert int(np.isinf(score).sum()) == int((counts < 2).sum()) > 100
    for tile, cap in ((16, INF), (8, 0.05), (32, float(np.median(score))), (64, INF)):
        got = film.score_tiles(tile, cap=cap)
        torch.cuda.synchronize()
        assert_planes(gpu.read_tile_scores(got), ref.tiles_ref(score, tile, cap), (tile, cap))
        assert tuple(got["mean"].shape) == (-(-H // tile), -(-W // tile))
    wide = gpu.score_window(dev(score), 2, "max").cpu().numpy()
    got = gpu.read_tile_scores(film.score_tiles(16, cap=1.0, dilate=2, planes=SUBSET))
    assert_planes(got, ref.tiles_ref(wide, 16, 1.0), "dilated", SUBSET)
    worst = film.score_tiles(16, planes=("max",))["max"]
    assert float(worst.max().item()) == INF      # a tile with a pixel nobody can judge yet


# ---------------------------------------------------------------- 12. the render loop
def run_sim(build, stem, *extra):
    out = subprocess.run([build.RENDER_SIM_BIN, "--width", "64", "--height", "48", "--spp", "4", "--iterations", "3", "--threads", "4",
                          "--adaptive-pixels", "--stop-metric", "stderr", "--stem", stem] + list(extra), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_render_loop_stops_when_no_tile_is_open(gpu, tmp_path):
    """statmc_render_sim --adaptive-pixels --stop-tiles on 64 x 48, three iterations.  A tolerance of 0 is never met: every
    iteration runs and prints its line.  The printed count of open tiles equals, at every iteration of every run, the restatement on
    the score of the statistics that iteration dumped; a run ends at the first iteration whose count is 0."""
    from statmc_amd import build, pfm
    import error_reference as err_ref
    import plan_reference as plan_ref
    build.build_tools()
    line = re.compile(r"^Tile rule: iteration (\d+), open tiles (\d+) / (\d+) of (\d+) x \4 pixels, mean of the relative standard error under (\S+) "
                      r"above (\S+): (met|open)$", re.M)

    def restated(stem, spp, tile, tol, cap):
        rd = lambda what: np.asarray(pfm.read_pfm("%s-%d-t0-b0-%s.pfm" % (stem, spp, what)))
        score = err_ref.error_scores_ref(rd("n").astype(np.int32), rd("film-mean"), rd("film-m2"), plan_ref.RELATIVE, 1e-3, None)
        mean = ref.tiles_ref(score, tile, cap)["mean"]
        return int((sum_ref.keys_of(mean) > ref.key_of(F32(tol))).sum()), mean

    def check(out, stem, tile, tol, cap):
        lines = line.findall(out)
        n_iter = len(re.findall(r"^Iteration: ", out, re.M))
        assert len(lines) == n_iter >= 1, out
        spps = [int(s) for s in re.findall(r"^%s-(\d+)-t0-b0-n\.pfm$" % re.escape(stem.split("/")[-1]), "\n".join(sorted(p.name for p in tmp_path.iterdir())), re.M)]
        assert len(spps) == n_iter
        means = []
        for k, spp in enumerate(sorted(spps)):
            n_open, mean = restated(stem, spp, tile, tol, cap)
            means.append(mean)
            it, got_open, n_tiles, t, _, _, verdict = lines[k]
            assert (int(it), int(got_open), int(n_tiles), int(t)) == (k + 1, n_open, mean.size, tile), (lines[k], n_open)
            assert verdict == ("met" if n_open == 0 else "open")
            assert (n_open == 0) == (k + 1 == n_iter) or (k + 1 == n_iter == 3), lines      # the run ends at the first iteration without an open tile
        return n_iter, means

    never = run_sim(build, str(tmp_path / "never"), "--stop-tiles", "16:0")
    n_iter, means = check(never, str(tmp_path / "never"), 16, 0.0, INF)
    assert n_iter == 3 and ": met" not in never and "Planned" in never
    once = run_sim(build, str(tmp_path / "once"), "--stop-tiles", "32:1e30:0.25")
    assert check(once, str(tmp_path / "once"), 32, 1e30, 0.25)[0] == 1 and "Planned" not in once
    # a tolerance between the worst tile of the first and of the second iteration: the run ends at the second
    worst = [float(m.max()) for m in means]
    assert worst[1] < worst[0] < INF
    tol = float(F32((worst[0] + worst[1]) / 2))
    twice = run_sim(build, str(tmp_path / "twice"), "--stop-tiles", "16:%.9g" % tol)
    assert check(twice, str(tmp_path / "twice"), 16, tol, INF)[0] == 2
    both = run_sim(build, str(tmp_path / "both"), "--stop-tiles", "16:1e30", "--stop-at", "0.95:0")      # both must hold
    assert len(re.findall(r"^Iteration: ", both, re.M)) == 3 and "Converged" not in both
    for bad in (["--stop-tiles", "16:1"], ["--adaptive-pixels", "--stop-tiles", "16"], ["--adaptive-pixels", "--stop-tiles", "12:1"],
                ["--adaptive-pixels", "--stop-tiles", "16:-1"], ["--adaptive-pixels", "--preview", "2", "--stop-tiles", "16:1"]):
        r = subprocess.run([build.RENDER_SIM_BIN, "--width", "16", "--height", "16"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--stop-tiles" in r.stderr, (bad, r.stderr)
