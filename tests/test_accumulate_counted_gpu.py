"""statmc_accumulate_counted / statmc_accumulate_tiles_counted on the GPU: a dense arena plus an int32 film image of per-pixel
sample counts leaves, per pixel, the bits statmc_accumulate_tiles leaves when that pixel is handed over as a 1 x 1 tile holding its
first c(p) = min(max(count, 0), S) samples.  Comparisons are bitwise on int32 views of every state image unless a test says
otherwise.

Every arena is allocated with 2 S planes while S is passed as the capacity, and every slot s >= c(p) -- planes S .. 2 S - 1
included -- holds a mix of NaN, +inf and the format's largest numbers: a kernel that folds a dead slot or clamps late fails by
its bits, and reads only memory that exists."""
import os
import subprocess

import numpy as np
import pytest

from test_records_gpu import (FILMS, KINDS, TYPES, States, assert_matches_the_oracle, bits, dev, prepass_of, run_tiles, same)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES_HALF = (1, 2, 3)          # indices into TYPES: everything but the radiance type
FORMATS = [(), FEATURES_HALF]
FORMAT_IDS = ["fp32", "features_half"]
VECTOR, ELEMENT = 1, 2             # statmc_debug_last_accumulate_counted


def expected_path(W, H):
    return VECTOR if (W * H) % 4 == 0 else ELEMENT       # (torch's allocations are 16-byte aligned)


def junk_like(rng, a):
    big = 65504.0 if a.dtype == np.float16 else 3e38
    return rng.choice(np.array([np.nan, np.inf, big], a.dtype), size=a.shape)


def live_values(rng, shape, half):
    """log-normal, a fifth exact zeros, one x 1000 value (make_samples' shape); a half arena holds values that are halves"""
    s = np.exp(rng.normal(0.0, 1.0, shape)).astype(np.float32)
    s[rng.random(shape) < 0.2] = 0.0
    if s.size:
        s.reshape(-1)[int(rng.integers(0, s.size))] *= np.float32(1000.0)
    return np.minimum(s, 60000.0).astype(np.float16) if half else s


def make_arenas(rng, W, H, S, counts, types=TYPES, half=()):
    """Per type [2 S, H, W, C]: slot s of pixel p is live iff s < min(max(counts[p], 0), S), everything else is junk."""
    npx = W * H
    c = np.clip(np.asarray(counts).reshape(-1), 0, S)
    live = np.arange(2 * S)[:, None] < c[None, :]
    out = []
    for i, k in enumerate(types):
        a = live_values(rng, (2 * S, npx, k[1]), i in half)
        a[~live] = junk_like(rng, a)[~live]
        out.append(a.reshape(2 * S, H, W, k[1]))
    return out


def as_records(arenas, counts, S):
    """The live samples as records in pixel order, ascending s inside a pixel: what run_tiles and the oracle comparison take."""
    npx = arenas[0].shape[1] * arenas[0].shape[2]
    c = np.clip(np.asarray(counts).reshape(-1), 0, S)
    live = (np.arange(S)[:, None] < c[None, :]).T                        # [npx, S]
    pixels = np.repeat(np.arange(npx, dtype=np.int32), c)
    samples = [np.ascontiguousarray(a[:S].reshape(S, npx, -1).transpose(1, 0, 2)[live].astype(np.float32)) for a in arenas]
    assert all(np.isfinite(s).all() for s in samples)
    return pixels, samples


def counts_tensor(counts, W, H, offset=False):
    """[H, W] int32 on the device; offset: the image starts 4 bytes into its allocation (4-byte but not 16-byte aligned)"""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(counts, np.int32).reshape(-1)).cuda()
    if not offset:
        return flat.view(H, W)
    buf = torch.zeros(W * H + 4, dtype=torch.int32, device="cuda:0")
    view = buf[1:1 + W * H]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4
    return view.view(H, W)


def formats_of(api, half, types=TYPES):
    return [api.SAMPLES_F16 if i in half else api.SAMPLES_F32 for i in range(len(types))] if half else None


def run_counted(api, St, arenas, S, counts, half=(), rows=None, offset=False, first=0):
    """planes [first, first + S) of the arenas as a batch of capacity S"""
    import torch
    d = [dev(a) for a in arenas]
    sts = [api.make_stat_type(d[i][first:first + S], St.st[i], k[2], k[3], prepass_into=St.pre(i)) for i, k in enumerate(St.types)]
    api.accumulate(St.W, St.H, sts, rows=rows, sample_formats=formats_of(api, half, St.types), sample_counts=counts_tensor(counts, St.W, St.H, offset))
    path = api.last_accumulate_counted()
    torch.cuda.synchronize()
    return path


def run_uncounted(api, St, arenas, S, half=(), rows=None):
    import torch
    d = [dev(a) for a in arenas]
    sts = [api.make_stat_type(d[i][:S], St.st[i], k[2], k[3], prepass_into=St.pre(i)) for i, k in enumerate(St.types)]
    api.accumulate(St.W, St.H, sts, rows=rows, sample_formats=formats_of(api, half, St.types))
    assert api.last_accumulate_counted() == 0
    torch.cuda.synchronize()


def ragged_counts(rng, npx, top=40):
    """0 .. 9 samples per pixel, about a fifth of the pixels at 0, one pixel at `top`"""
    counts = rng.integers(1, 10, npx).astype(np.int32)
    counts[rng.random(npx) < 0.2] = 0
    counts[int(rng.integers(0, npx))] = top
    return counts


@pytest.fixture(scope="module", params=FILMS, ids=lambda f: "%dx%d" % f)
def ragged(request, gpu):
    """One ragged case per film, with the 1 x 1-tile yardstick's result, shared by the tests that need one."""
    W, H = request.param
    rng = np.random.default_rng(2000 + W)
    S = 40
    counts = ragged_counts(rng, W * H)
    arenas = make_arenas(rng, W, H, S, counts)
    pixels, samples = as_records(arenas, counts, S)
    B = States(W, H)
    run_tiles(gpu, B, pixels, samples)
    return W, H, S, counts, arenas, B.snapshot()


@pytest.mark.parametrize("half", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_uniform_counts_equal_the_uncounted_entry(gpu, film, half):
    W, H = film
    S = 7
    rng = np.random.default_rng(17 + W)
    A, B = States(W, H), States(W, H)
    for batch in range(2):                       # the second batch continues a non-zero state
        counts = np.full(W * H, S, np.int32)
        arenas = make_arenas(rng, W, H, S, counts, half=half)
        assert run_counted(gpu, A, arenas, S, counts, half=half) == expected_path(W, H)
        run_uncounted(gpu, B, arenas, S, half=half)
    assert int(A.st[0]["n"].min()) == int(A.st[0]["n"].max()) == 2 * S
    same(A.snapshot(), B.snapshot())


def test_ragged_counts_equal_the_one_pixel_tiles(gpu, ragged):
    W, H, S, counts, arenas, want = ragged
    assert (counts == 0).mean() > 0.1 and counts.max() == S
    A = States(W, H)
    assert run_counted(gpu, A, arenas, S, counts) == expected_path(W, H)      # a counted kernel, on the path the film calls for
    assert np.array_equal(A.st[0]["n"].cpu().numpy().reshape(-1), counts)
    same(A.snapshot(), want)
    if expected_path(W, H) == VECTOR:            # the counts image 4 bytes off: element by element, the same bits
        A = States(W, H)
        assert run_counted(gpu, A, arenas, S, counts, offset=True) == ELEMENT
        same(A.snapshot(), want)
    A = States(W, H)                             # ... and on every run
    run_counted(gpu, A, arenas, S, counts)
    same(A.snapshot(), want)


def test_pixels_with_count_zero_keep_every_bit(gpu, ragged):
    W, H, S, counts, arenas, _ = ragged
    St = States(W, H, fill=np.random.default_rng(5))          # a seeded bit pattern everywhere, mean_corr / discriminator included
    for st in St.st:
        st["n"].remainder_(1000).abs_()
    before = St.snapshot()
    run_counted(gpu, St, arenas, S, counts)
    after = St.snapshot()
    untouched = counts == 0
    assert untouched.any()
    for x, y in zip(before, after):
        xs, ys = x.reshape(W * H, -1), y.reshape(W * H, -1)
        assert np.array_equal(xs[untouched], ys[untouched])
    assert np.array_equal(after[0].reshape(-1) - before[0].reshape(-1), counts)
    run_counted(gpu, St, arenas, S, np.zeros(W * H, np.int32))                    # all counts 0: nothing changes anywhere
    same(after, St.snapshot())
    run_counted(gpu, St, arenas, 0, counts)                                       # capacity 0: a no-op
    same(after, St.snapshot())


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_counts_outside_the_capacity_are_clamped(gpu, film):
    W, H = film
    S = 6
    rng = np.random.default_rng(31 + W)
    counts = rng.integers(-S, 2 * S + 1, W * H).astype(np.int32)
    counts[:4] = [-2 ** 31, 2 ** 31 - 1, -1, 2 * S]
    assert (counts < 0).any() and (counts > S).any()
    arenas = make_arenas(rng, W, H, S, counts)                 # junk from the CLAMPED count on, planes S .. 2 S - 1 included
    A, B = States(W, H), States(W, H)
    run_counted(gpu, A, arenas, S, counts)
    run_counted(gpu, B, arenas, S, np.clip(counts, 0, S))
    assert np.array_equal(A.st[0]["n"].cpu().numpy().reshape(-1), np.clip(counts, 0, S))
    same(A.snapshot(), B.snapshot())
    pixels, samples = as_records(arenas, counts, S)
    C = States(W, H)
    run_tiles(gpu, C, pixels, samples)
    same(A.snapshot(), C.snapshot())


@pytest.mark.parametrize("offset", [False, True], ids=["vector", "element"])
def test_every_kind_at_ragged_counts_matches_the_oracle(gpu, oracle, offset):
    """All twelve (channels, transform, max_moment) kinds in one call, test_every_kind_at_the_walks_edges_matches_the_oracle's comparison."""
    W, H, S = 16, 8, 17
    rng = np.random.default_rng(43)
    counts = np.resize(np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17], np.int32), W * H)
    arenas = make_arenas(rng, W, H, S, counts, types=KINDS)
    pixels, samples = as_records(arenas, counts, S)
    St = States(W, H, types=KINDS)
    assert run_counted(gpu, St, arenas, S, counts, offset=offset) == (ELEMENT if offset else VECTOR)
    assert_matches_the_oracle(oracle, St, counts, pixels, samples)


@pytest.mark.parametrize("spec", ["default", "welch_exclude"])
def test_epilogue_is_statmc_prepass(gpu, ragged, spec):
    api = gpu
    W, H, S, counts, arenas, _ = ragged
    try:
        if spec == "welch_exclude":
            api.set_filter_spec(dof=api.DOF_WELCH, small_n=1)
        else:
            api.set_filter_spec()
        St = States(W, H)
        St.mc.fill_(7.0)
        St.dc.fill_(7.0)
        run_counted(api, St, arenas, S, counts)
        mc, dc = prepass_of(api, St.st[0], 3)
        touched = (counts > 0).reshape(H, W)
        assert (counts == 1).any()               # n = 1: the small-n branch
        for got, want in ((St.mc, mc), (St.dc, dc)):
            g, w = bits(got), bits(want)
            assert np.array_equal(g[touched], w[touched])
            assert (g[~touched] == np.float32(7.0).view(np.int32)).all()      # pixels without a live sample keep what was there
    finally:
        api.set_filter_spec()


def test_row_ranges(gpu, ragged):
    W, H, S, counts, arenas, _ = ragged
    ranges = [(2, 9), (15, 20)]
    fill = lambda: States(W, H, fill=np.random.default_rng(9))
    A, B = fill(), fill()
    for St in (A, B):
        for st in St.st:
            st["n"].remainder_(1000).abs_()
    before = A.snapshot()
    run_counted(gpu, A, arenas, S, counts, rows=ranges)
    run_counted(gpu, B, arenas, S, counts)
    inside = np.zeros((H, W), bool)
    for y0, y1 in ranges:
        inside[y0:y1] = True
    inside = inside.reshape(-1)
    for x, y, z in zip(before, A.snapshot(), B.snapshot()):
        xs, ys, zs = (v.reshape(W * H, -1) for v in (x, y, z))
        assert np.array_equal(ys[inside], zs[inside])            # the whole-film call on those rows
        assert np.array_equal(ys[~inside], xs[~inside])          # rows outside the ranges keep every bit


@pytest.mark.parametrize("k", [1, 4])
def test_split_along_s_equals_one_call(gpu, ragged, k):
    W, H, S, counts, arenas, want = ragged
    A = States(W, H)
    run_counted(gpu, A, arenas, k, np.minimum(counts, k))
    run_counted(gpu, A, arenas, S - k, np.maximum(counts - k, 0), first=k)
    same(A.snapshot(), want)


# ------------------------------------------------------------------ the tile entry
def tile_case(rng, W, H, half, all_live=False, T=16):
    """T x T tiles clipped to the film; tile_samples in {0, 3, 12}; a block holds 2 tile_samples planes (the second half junk) and
    there is slack behind the last block.  Returns the tables, the counts image, the flat arenas and the live samples as records."""
    bounds = np.array([(x, y, min(x + T, W), min(y + T, H)) for y in range(0, H, T) for x in range(0, W, T)], np.int32)
    n_tiles = len(bounds)
    ts = np.resize(np.array([3, 12, 0, 12, 3], np.int32), n_tiles)
    rng.shuffle(ts)
    npx_k = (bounds[:, 2] - bounds[:, 0]) * (bounds[:, 3] - bounds[:, 1])
    sizes = 2 * ts.astype(np.int64) * npx_k
    offsets = (np.cumsum(sizes) - sizes).astype(np.int64)
    total = int(sizes.sum()) + 64
    counts = np.zeros((H, W), np.int32)
    flat = []
    for i, k in enumerate(TYPES):
        a = np.zeros((total, k[1]), np.float16 if i in half else np.float32)
        a[:] = junk_like(rng, a)
        flat.append(a)
    pixels, samples = [], [[] for _ in TYPES]
    for t, (x0, y0, x1, y1) in enumerate(bounds):
        th, tw, cap = y1 - y0, x1 - x0, int(ts[t])
        if all_live:
            c = cap + rng.integers(0, 3, (th, tw))
        else:
            c = rng.integers(0, cap + 1, (th, tw))
            c[rng.random((th, tw)) < 0.1] = cap + 5              # above the capacity
            c[rng.random((th, tw)) < 0.05] = -3
        counts[y0:y1, x0:x1] = c
        live = np.arange(2 * cap)[:, None, None] < np.clip(c, 0, cap)[None]          # [2 cap, th, tw]
        film_px = ((y0 + np.arange(th))[:, None] * W + x0 + np.arange(tw)[None, :]).astype(np.int32)
        pixels.append(np.broadcast_to(film_px[None], live.shape)[live])
        for i, k in enumerate(TYPES):
            block = flat[i][offsets[t]:offsets[t] + sizes[t]].reshape(2 * cap, th, tw, k[1])
            vals = live_values(rng, block.shape, i in half)
            block[live] = vals[live]
            samples[i].append(block[live].astype(np.float32))
    pixels = np.concatenate(pixels)
    samples = [np.ascontiguousarray(np.concatenate(s)) for s in samples]
    return bounds, offsets, ts, counts, flat, pixels, samples


def run_tiles_counted(api, St, case, half, counted=True):
    import torch
    bounds, offsets, ts, counts, flat, _, _ = case
    arenas = [dev(a.reshape(-1)) for a in flat]
    sts = [api.make_stat_type_arena(arenas[i], k[1], St.st[i], k[2], k[3], prepass_into=St.pre(i)) for i, k in enumerate(TYPES)]
    api.accumulate_tiles(St.W, St.H, sts, dev(bounds), dev(offsets), dev(ts), sample_formats=formats_of(api, half),
                         sample_counts=counts_tensor(counts, St.W, St.H) if counted else None)
    path = api.last_accumulate_counted()
    torch.cuda.synchronize()
    return path


@pytest.mark.parametrize("half", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("film", [(96, 48), (37, 29)], ids=lambda f: "%dx%d" % f)
def test_tile_entry_equals_the_one_pixel_tiles(gpu, film, half):
    W, H = film
    case = tile_case(np.random.default_rng(50 + W), W, H, half)
    ts, counts = case[2], case[3]
    assert set(ts.tolist()) == {0, 3, 12} and (counts > 12).any() and (counts < 0).any()
    A, B = States(W, H), States(W, H)
    assert run_tiles_counted(gpu, A, case, half) == expected_path(W, H)
    run_tiles(gpu, B, case[5], case[6])
    same(A.snapshot(), B.snapshot())


@pytest.mark.parametrize("half", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("film", [(96, 48), (37, 29)], ids=lambda f: "%dx%d" % f)
def test_tile_entry_with_full_counts_equals_the_uncounted_entry(gpu, film, half):
    W, H = film
    case = tile_case(np.random.default_rng(60 + W), W, H, half, all_live=True)
    A, B = States(W, H), States(W, H)
    assert run_tiles_counted(gpu, A, case, half) != 0
    assert run_tiles_counted(gpu, B, case, half, counted=False) == 0
    same(A.snapshot(), B.snapshot())


def test_film_stats_takes_counts(gpu):
    """FilmStats.accumulate(samples, counts=): the bits of api.accumulate with sample_counts."""
    import torch
    from statmc_amd.film import STAT_TYPES, FilmStats
    W, H, S = 64, 32, 5
    rng = np.random.default_rng(77)
    counts = rng.integers(0, S + 1, (H, W)).astype(np.int32)
    names = ("radiance", "normal", "depth")
    film = FilmStats(W, H, torch.device("cuda:0"), types=names, g_buffers=("normal",))
    smp = {t: dev(live_values(rng, (S, H, W, STAT_TYPES[t]["channels"]), False)) for t in names}
    film.accumulate(smp, counts=dev(counts))
    assert gpu.last_accumulate_counted() == VECTOR
    torch.cuda.synchronize()
    assert np.array_equal(film.state["radiance"]["n"].cpu().numpy(), counts)
    want = {t: {k: torch.zeros_like(v) for k, v in film.state[t].items() if v is not None} for t in names}
    sts = [gpu.make_stat_type(smp[t], want[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"]) for t in names]
    gpu.accumulate(W, H, sts, sample_counts=dev(counts))
    torch.cuda.synchronize()
    for t in names:
        for k, v in want[t].items():
            assert np.array_equal(bits(film.state[t][k]), bits(v)), (t, k)
    with pytest.raises(ValueError):
        film.accumulate(smp, counts=dev(counts[:-1]))


def test_estimator_ragged_tiles_equal_accumulate_records(gpu):
    """C++ host: an Estimator fed ragged StatTiles through Merge[Transform]Tiles holds the bits of one fed the same samples, ordered by
    s, through AccumulateRecords and of one fed the dense arena and the count image through AccumulateFilm; a flush of only uniform
    tiles stages no counts and leaves the same bits too (tests/cpp/test_accumulate_counted.cpp)."""
    from statmc_amd import build
    build.build_tools()
    for w, h in ((61, 37), (96, 64)):
        out = subprocess.run([build.ACC_COUNTED_BIN, str(w), str(h)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "accumulate counted ok" in out.stdout
