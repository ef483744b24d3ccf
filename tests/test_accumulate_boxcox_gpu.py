"""The Box-Cox moments of the accumulation, element by element.  Wherever the transform is on, the rest of the suite holds
`mean` / `m2` / `m3` to the oracle by relative L2 over the whole image (the device takes v_sqrt_f32 where the oracle takes pow):
one wrong pixel, or an error shared by add_sample and add_sample2, passes there.  Here the comparison is split into two exact
halves (tests/test_accumulate_boxcox_cpu.py has the yardsticks and their own tests):
  (a) the device's Box-Cox value v of every sample -- read through the public entry, one sample folded into a zeroed state leaves
      mean = v -- is one of the floats a root within 1 ulp allows, the same at every fold site;
  (b) given the device's own v, `mean` / `m2` / `m3` are the oracle's untransformed chain on v, bit for bit (NaN matching NaN),
      from a host-made starting state, for every entry that folds samples: statmc_accumulate (vector walk with uniform and ragged
      counts, scalar walk, row ranges), statmc_accumulate_tiles, the type-fused walk in fp32 and half, statmc_accumulate_records
      and the fused interleaved records kernel.  film_mean / film_m2 stay with the transform=True oracle, and an epilogue's
      mean_corr / disc with oracle.prepass of the stored moments, both bit for bit.
An infinite sample: the division by the count leaves NaN for an infinite dividend where the reference leaves inf
(include/statmc.h).  The read-out of v goes through that division, so it returns NaN for +inf (asserted), the chain on the values
read holds NaN like the device, and film_mean / film_m2 of such an element are asserted NaN here and non-finite in the oracle.

Out of scope here, each tied bit for bit to an entry anchored above by a test of its own:
  the split records entries (statmc_accumulate_records_split, ..._interleaved_split): their definition contains the fp32 combine;
      tests/test_records_split_gpu.py holds them bit for bit to statmc_accumulate_records per chunk and statmc_combine_statistics
      per tree edge, tests/test_records_split_cpu.py has their float64 yardstick;
  the device-API example library (PixelStats in a renderer's kernel): tests/test_device_api_gpu.py, against statmc_accumulate;
  merge_lanes / merge_waves: tests/test_device_reduce_gpu.py, against statmc_combine_statistics in the tree's order;
  statmc_accumulate_records_interleaved through the general kernel: tests/test_records_interleaved_gpu.py, against
      statmc_accumulate_records."""
import numpy as np
import pytest
import torch

from test_accumulate_boxcox_cpu import (box_cox_candidates, chain_reference, directed_samples, f32_bits, heavy_tailed_samples, in_candidates,
                                        infinite_sample_elements, nearest_box_cox, oracle_box_cox, random_start_state, same_bits_or_nan)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANES = ("mean", "m2", "m3", "film_mean", "film_m2")
RAGGED_AT = (1, 41)       # 256 x 4: the second wave of the workgroup (tests/test_accumulate_fused_sets_gpu.py)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_state(st):
    return {k: to_dev(v) for k, v in st.items()}


def host(st):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}


def zero_state(H, W, c):
    z = lambda: torch.zeros(H, W, c, dtype=torch.float32, device=DEV)
    return dict(n=torch.zeros(H, W, dtype=torch.int32, device=DEV), mean=z(), m2=z(), m3=z(), film_mean=z(), film_m2=z())


# ------------------------------------------------------------------ (a) reading v
def device_box_cox(gpu, samples, via="aligned"):
    """The device's Box-Cox value of every sample (any shape, float32; the same shape back): a one-channel film with one sample per
    pixel (padded with 1.0), folded into a zeroed state with max_moment 1 and the transform on; `mean` is v.  via: the fold site --
      aligned  256 wide, 16-byte aligned planes: the vector walk from a uniform count, add_sample2 (the packed fma(root, 2, -2));
      odd      37 wide with a pixel count that is no multiple of 4: accumulate_pixel -> add_sample ((root - 1) / .5 in two steps);
      records  statmc_accumulate_records, one record per pixel: PixelStats::add -> add_sample;
      half     a half arena through statmc_accumulate_formats (the samples must be half values): the 16-bit vector loader."""
    smp = np.ascontiguousarray(samples, np.float32).reshape(-1)
    if smp.size == 0:
        return smp.reshape(np.shape(samples))
    W = 37 if via == "odd" else 256
    H = -(-smp.size // W)
    if via == "odd" and (W * H) % 4 == 0:
        H += 1
    assert 0 < H < 65536
    film = np.ones(W * H, np.float32)
    film[:smp.size] = smp
    st = zero_state(H, W, 1)
    assert all(v.data_ptr() % 16 == 0 for v in st.values())
    if via == "records":
        d, d_px = to_dev(film.reshape(-1, 1)), to_dev(np.arange(W * H, dtype=np.int32))
        gpu.accumulate_records(W, H, [gpu.make_stat_type_records(d, 1, st, True, 1)], d_px)
    elif via == "half":
        h = film.astype(np.float16)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(h.astype(np.float32), film, equal_nan=True), "the half site takes half-representable samples"
        d = to_dev(h.reshape(1, H, W, 1))
        gpu.accumulate(W, H, [gpu.make_stat_type(d, st, True, 1)], sample_formats=[gpu.SAMPLES_F16])
        assert gpu.last_accumulate_fused() == 0 and gpu.last_accumulate_loader() == 1, "the 16-bit vector loader"
    else:
        d = to_dev(film.reshape(1, H, W, 1))
        assert d.data_ptr() % 16 == 0 and ((W * H) % 4 == 0) == (via == "aligned")      # what the plan's `vec` asks of an fp32 type
        gpu.accumulate(W, H, [gpu.make_stat_type(d, st, True, 1)])
        assert gpu.last_accumulate_fused() == 0 and gpu.last_accumulate_loader() == 0
    got = host(st)
    raw = np.where(np.isinf(film), np.float32(np.nan), film)     # (an infinite sample over the count 1: NaN, see the module docstring)
    assert (got["n"] == 1).all() and np.array_equal(got["film_mean"].reshape(-1), raw, equal_nan=True)
    assert not got["m2"].any() and not got["m3"].any()
    return got["mean"].reshape(-1)[:smp.size].reshape(np.shape(samples))


def test_transform_per_sample_at_every_fold_site(gpu, oracle):
    """About 78 000 directed samples in one launch per site: all four sites return the same bits, every value is one a root
    within 1 ulp allows, exact squares are exact.  Prints how many values are not the correctly rounded root's (a measurement:
    DESIGN.md 4.1 records it)."""
    smp = directed_samples()
    exact = box_cox_candidates(smp)[1]
    v = {via: device_box_cox(gpu, smp, via) for via in ("aligned", "odd", "records")}
    for via in ("odd", "records"):
        same_bits_or_nan(v[via], v["aligned"], "v through %s against aligned" % via, channels=1)
    # the half site: every non-negative half there is, the infinity and the NaNs included, and -0, -1 and -inf
    halves = np.concatenate([np.arange(0, 0x8000, dtype=np.uint16), np.array([0x8000, 0xBC00, 0xFC00], np.uint16)]).view(np.float16).astype(np.float32)
    v_half, v_wide = device_box_cox(gpu, halves, "half"), device_box_cox(gpu, halves, "aligned")
    same_bits_or_nan(v_half, v_wide, "v through half against aligned", channels=1)
    for what, s_, v_ in (("directed", smp, v["aligned"]), ("halves", halves, v_wide)):
        c_, exact_ = box_cox_candidates(s_)
        inf_s = np.isposinf(s_)
        assert inf_s.sum() == 1 and np.isnan(v_[inf_s]).all(), (what, "+inf over the count 1 reads NaN")
        ok = in_candidates(v_, c_) | inf_s
        assert ok.all(), "%s: %d values outside what a 1-ulp root allows; the first: sample %r (0x%08x) -> %r, allowed %r" % (
            what, int((~ok).sum()), float(s_[~ok][0]), int(f32_bits(s_[~ok][0]).reshape(-1)[0]) & 0xffffffff, float(v_[~ok][0]), c_[~ok][0].tolist())
        sq = exact_ & ~inf_s
        assert sq.sum() >= 127 and (f32_bits(v_[sq]) == f32_bits(c_[sq, 0])).all(), (what, "exact squares are exact")
    assert exact.sum() >= 4096 + 127
    pos = np.isfinite(smp) & (smp > 0)
    off = f32_bits(v["aligned"][pos]) != f32_bits(nearest_box_cox(smp[pos]))
    rng = np.random.default_rng(99)
    logn = rng.lognormal(0, 2.5, 7680).astype(np.float32)
    v_dev, v_or, v_near = device_box_cox(gpu, logn), oracle_box_cox(oracle, logn), nearest_box_cox(logn)
    assert in_candidates(v_dev, box_cox_candidates(logn)[0]).all()
    print("\nBox-Cox values that are not the correctly rounded root's: device %d of %d directed samples; of 7680 lognormal(0, 2.5) samples device %d, oracle %d"
          % (int(off.sum()), int(pos.sum()), int((f32_bits(v_dev) != f32_bits(v_near)).sum()), int((f32_bits(v_or) != f32_bits(v_near)).sum())))


# ------------------------------------------------------------------ (b) the chain
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def shared_inputs():
    """Samples and the v read from the device are computed once per sample set and shared, read only."""
    yield
    _CACHE.clear()


def sample_set(gpu, key, S, H, W, c, half=False):
    """(samples [S, H, W, c] on the host, the device's v of them): the heavy-tailed recipe, v read with one launch (half: through
    the half site)."""
    key = (key, S, H, W, c, half)
    if key not in _CACHE:
        rng = np.random.default_rng(7919 * S + 131 * H + 17 * W + c + sum(map(ord, key[0])) + (1000003 if half else 0))
        smp = heavy_tailed_samples(rng, S, H, W, c, half=half)
        v = device_box_cox(gpu, smp, "half" if half else "aligned")
        assert np.isnan(v).sum() == 2 and not np.isinf(v).any()      # the negative sample and the infinite one
        _CACHE[key] = (smp, v)
    return _CACHE[key]


def start_counts(H, W, count, ragged):
    n = np.full((H, W), count, np.int32)
    if ragged == "one":                                           # one pixel two samples ahead: its wave takes the element-by-element walk
        n[RAGGED_AT] += 2
    elif ragged == "all":
        n = np.random.default_rng(H * 1000 + W).integers(0, 40, (H, W)).astype(np.int32)
    return n


def over_rows(fn, state, arrays, rows, H):
    """fn(sub_state, *sub_arrays) on the rows of the launch ([S, H, W, C] arrays cut along H); the other rows keep the start."""
    out = {k: v.copy() for k, v in state.items()}
    for y0, y1 in (rows if rows is not None else [(0, H)]):
        part = fn({k: np.ascontiguousarray(v[y0:y1]) for k, v in out.items()}, *[np.ascontiguousarray(a[:, y0:y1]) for a in arrays])
        for k, v in part.items():
            out[k][y0:y1] = v
    return out


def assert_chain(oracle, what, start, got, ref_chain, ref_film, s_inf, mm, prepass=None, pre_rows=None):
    """got (host arrays after the launch) against the two oracle runs; s_inf [H, W, C]: the elements handed an infinite sample."""
    assert np.array_equal(got["n"], ref_chain["n"]), (what, "n")
    for k in ("mean", "m2", "m3"):
        if k not in ("mean", "m2", "m3")[:mm]:                      # moments above max_moment keep every bit
            assert np.array_equal(f32_bits(ref_chain[k]), f32_bits(start[k])), (what, k)
        else:
            assert np.isnan(got[k][s_inf]).all(), (what, k, "elements handed an infinite sample")
        same_bits_or_nan(got[k], ref_chain[k], "%s: %s" % (what, k))
    for k in ("film_mean", "film_m2"):
        g, ref = got[k].copy(), ref_film[k].copy()
        assert np.isnan(g[s_inf]).all() and not np.isfinite(ref[s_inf]).any(), (what, k, "elements handed an infinite sample")
        g[s_inf] = ref[s_inf] = np.nan
        same_bits_or_nan(g, ref, "%s: %s" % (what, k))
    if prepass is not None:
        mc, dc = (x.cpu().numpy() for x in prepass)
        mc_ref, dc_ref = oracle.prepass(got["n"], got["mean"], got["m2"], got["m3"])
        for y0, y1 in (pre_rows if pre_rows is not None else [(0, got["n"].shape[0])]):
            same_bits_or_nan(mc[y0:y1], mc_ref[y0:y1], "%s: mean_corr rows %d..%d" % (what, y0, y1))
            same_bits_or_nan(dc[y0:y1], dc_ref[y0:y1], "%s: disc rows %d..%d" % (what, y0, y1))


def run_accumulate(gpu, oracle, what, smp, v, c, mm, n0, rows=None, seed=0):
    """statmc_accumulate (rows: statmc_accumulate_rows) of a transformed type from a host-made state, both halves of the check."""
    S, H, W, _ = smp.shape
    start = random_start_state(np.random.default_rng(1234 + seed), H, W, c, n0)
    st = dev_state(start)
    pre = (torch.full((H, W, c), 3.0, device=DEV), torch.full((H, W, c), 3.0, device=DEV)) if mm == 3 else None
    d_smp = to_dev(smp)                                             # (held: the descriptor has its address only)
    gpu.accumulate(W, H, [gpu.make_stat_type(d_smp, st, True, mm, prepass_into=pre)], rows=rows)
    assert gpu.last_accumulate_fused() == 0 and gpu.last_accumulate_loader() == 0, what
    got = host(st)
    rr = [tuple(rows)] if rows is not None else None
    ref_chain = over_rows(lambda sub, a: oracle.accumulate(sub, a, False, mm), start, [v], rr, H)
    ref_film = over_rows(lambda sub, a: oracle.accumulate(sub, a, True, mm), start, [smp], rr, H)
    s_inf = np.zeros((H, W, c), bool)
    for y0, y1 in (rr or [(0, H)]):
        s_inf[y0:y1] = infinite_sample_elements(smp[:, y0:y1])
    assert rows is not None or s_inf.sum() == 1
    assert_chain(oracle, what, start, got, ref_chain, ref_film, s_inf, mm, prepass=pre, pre_rows=rr)
    if rows is not None:                                            # rows outside keep every bit of the start, the epilogue's images too
        out = np.ones(H, bool)
        out[rows[0]:rows[1]] = False
        for k in PLANES + ("n",):
            assert np.array_equal(got[k][out].view(np.int32), start[k][out].view(np.int32)), (what, k, "rows outside the launch")
        if pre is not None:
            assert all(bool((x[torch.from_numpy(out).to(DEV)] == 3.0).all()) for x in pre), (what, "epilogue outside the rows")
    return got


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("max_moment", [1, 2, 3])
def test_accumulate_vector_walk(gpu, oracle, channels, max_moment):
    """256 x 4, one workgroup: batches below, at and above the ring depth (3) and the unroll (a U-multiple plus a remainder), from
    a uniform count (the shared-reciprocal packed walk, add_sample2) and with one pixel two samples ahead (its wave folds element
    by element, add_sample)."""
    for S in (1, 3, 4, 17):
        smp, v = sample_set(gpu, "vec", S, 4, 256, channels)
        for ragged in (None, "one"):
            run_accumulate(gpu, oracle, "aligned c%d m%d S=%d ragged=%s" % (channels, max_moment, S, ragged), smp, v, channels, max_moment,
                           start_counts(4, 256, 2, ragged), seed=S)


@pytest.mark.parametrize("channels,max_moment", [(1, 3), (3, 3), (3, 1), (1, 2)])
def test_accumulate_scalar_walk(gpu, oracle, channels, max_moment):
    """37 x 23: 851 pixels, no multiple of 4 -- every pixel through accumulate_pixel, from ragged counts."""
    smp, v = sample_set(gpu, "scalar", 5, 23, 37, channels)
    run_accumulate(gpu, oracle, "scalar c%d m%d" % (channels, max_moment), smp, v, channels, max_moment, start_counts(23, 37, 0, "all"))


@pytest.mark.parametrize("channels,max_moment", [(3, 3), (1, 2)])
def test_accumulate_row_range(gpu, oracle, channels, max_moment):
    """100 x 5, rows 1 .. 3 through statmc_accumulate_rows: 75 groups, the last wave partial; the rows outside keep every bit."""
    smp, v = sample_set(gpu, "rows", 6, 5, 100, channels)
    for ragged in (None, "all"):
        run_accumulate(gpu, oracle, "rows c%d m%d ragged=%s" % (channels, max_moment, ragged), smp, v, channels, max_moment,
                       start_counts(5, 100, 3, ragged), rows=(1, 4))


@pytest.mark.parametrize("W,H", [(64, 40), (50, 37)], ids=["vector-tiles", "scalar-tiles"])
def test_accumulate_tiles(gpu, oracle, W, H):
    """statmc_accumulate_tiles, the radiance type: the shapes and tile lists of test_gpu_parity.test_accumulate_tiles_matches_oracle
    (16 x 16 tiles in shuffled order, a different sample count per tile, some empty; two iterations) from a ragged host-made state."""
    rng = np.random.default_rng(W * 1000 + H)
    start = random_start_state(rng, H, W, 3, rng.integers(0, 30, (H, W)))
    st = dev_state(start)
    pre = (torch.full((H, W, 3), 3.0, device=DEV), torch.full((H, W, 3), 3.0, device=DEV))
    ref_chain, ref_film = ({k: a.copy() for k, a in start.items()} for _ in range(2))
    v_inf, touched = np.zeros((H, W, 3), bool), np.zeros((H, W), bool)
    tiles = [(x, y, min(x + 16, W), min(y + 16, H)) for y in range(0, H, 16) for x in range(0, W, 16)]
    for it in range(2):
        order = rng.permutation(len(tiles))
        counts = rng.choice([0, 1, 3, 7, 12], size=len(tiles))
        counts[order[0]] = 7                                                      # (the planted samples need a tile with samples)
        blocks, shapes, offsets, off = [], [], [], 0
        for k in order:
            x0, y0, x1, y1 = tiles[k]
            S, npx = int(counts[k]), (x1 - x0) * (y1 - y0)
            size = (S * npx + 3) // 4 * 4                                         # blocks start on 4-pixel-sample boundaries
            blk = np.zeros(size * 3, np.float32)
            if S:
                blk[:S * npx * 3] = heavy_tailed_samples(rng, S, y1 - y0, x1 - x0, 3).ravel() if k == order[0] else \
                    (rng.lognormal(0, 2.5, size=S * npx * 3) * (rng.random(S * npx * 3) >= 0.15)).astype(np.float32)
            blocks.append(blk)
            shapes.append((S, y1 - y0, x1 - x0, 3))
            offsets.append(off)
            off += size
        arena = np.concatenate(blocks)
        v_arena = device_box_cox(gpu, arena)
        bounds = [tiles[k] for k in order]
        d_arena = to_dev(arena)                                                    # (held: the descriptor has its address only)
        t = gpu.make_stat_type_arena(d_arena, 3, st, True, 3, prepass_into=pre)
        gpu.accumulate_tiles(W, H, [t], to_dev(np.array(bounds, np.int32)), to_dev(np.array(offsets, np.int64)), to_dev(counts[order].astype(np.int32)))
        torch.cuda.synchronize()
        for (x0, y0, x1, y1), o, shp in zip(bounds, offsets, shapes):
            if shp[0]:
                touched[y0:y1, x0:x1] = True
                for ref, src, tr in ((ref_chain, v_arena, False), (ref_film, arena, True)):
                    sub = {key: np.ascontiguousarray(a[y0:y1, x0:x1]) for key, a in ref.items()}
                    oracle.accumulate(sub, np.ascontiguousarray(src[3 * o:3 * o + int(np.prod(shp))].reshape(shp)), tr, 3)
                    for key, a in sub.items():
                        ref[key][y0:y1, x0:x1] = a
                v_inf[y0:y1, x0:x1] |= infinite_sample_elements(arena[3 * o:3 * o + int(np.prod(shp))].reshape(shp))
    assert 1 <= v_inf.sum() <= 2
    got = host(st)
    assert_chain(oracle, "tiles %dx%d" % (W, H), start, got, ref_chain, ref_film, v_inf, 3)
    # the epilogue writes the tiles that handed samples over (in either launch: the moments have not changed since), nothing else
    mc_ref, dc_ref = oracle.prepass(got["n"], got["mean"], got["m2"], got["m3"])
    for img, ref, name in ((pre[0], mc_ref, "mean_corr"), (pre[1], dc_ref, "disc")):
        img = img.cpu().numpy()
        same_bits_or_nan(img[touched], ref[touched], "tiles %dx%d: %s" % (W, H, name), channels=3)
        assert (img[~touched] == 3.0).all(), name


ALL = ("radiance", "normal", "albedo", "depth", "materialid")


@pytest.mark.parametrize("fmt", ["fp32", "all_half"])
def test_fused_walk(gpu, oracle, fmt):
    """The type-fused walk of all five types (set K = 2, M = 2) at 256 x 4, four samples, the switch at 1: the radiance branch of
    accumulate_fused_kernel / accumulate_fused_half_kernel.  all_half: the samples are half values and v is read through the half
    site.  The feature types' means against the oracle bit for bit, as everywhere."""
    from statmc_amd import film
    W, H, S = 256, 4, 4
    half = fmt == "all_half"
    rng = np.random.default_rng(55)
    smp, v, start, st, sts, keep = {}, None, {}, {}, [], []
    pre = (torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 3, device=DEV))
    for t in ALL:
        cfg = film.STAT_TYPES[t]
        if t == "radiance":
            smp[t], v = sample_set(gpu, "fused", S, H, W, 3, half=half)
        else:
            smp[t] = rng.random((S, H, W, cfg["channels"]), dtype=np.float32)
            if half:
                smp[t] = smp[t].astype(np.float16).astype(np.float32)
        start[t] = random_start_state(rng, H, W, cfg["channels"], start_counts(H, W, 2 + ALL.index(t), None))
        if not cfg["transform"]:
            start[t]["film_mean"], start[t]["film_m2"] = start[t]["mean"].copy(), start[t]["m2"].copy()
        st[t] = dev_state(start[t])
        d = to_dev(smp[t].astype(np.float16) if half else smp[t])
        keep.append(d)
        sts.append(gpu.make_stat_type(d, st[t], cfg["transform"], cfg["max_moment"], prepass_into=pre if t == "radiance" else None))
    try:
        gpu.accumulate_fused(1)
        gpu.accumulate(W, H, sts, sample_formats=[gpu.SAMPLES_F16] * len(ALL) if half else None)
        assert gpu.last_accumulate_fused() == 1 and gpu.last_accumulate_loader() == (1 if half else 0)
    finally:
        gpu.accumulate_fused(0)
    for t in ALL:
        cfg = film.STAT_TYPES[t]
        got = host(st[t])
        if t == "radiance":
            ref_chain = chain_reference(oracle, start[t], v, 3)
            ref_film = oracle.accumulate({k: a.copy() for k, a in start[t].items()}, smp[t], True, 3)
            assert_chain(oracle, "fused %s" % fmt, start[t], got, ref_chain, ref_film, infinite_sample_elements(smp[t]), 3, prepass=pre)
        else:
            ref = oracle.accumulate({k: a.copy() for k, a in start[t].items()}, smp[t], False, 1)
            assert np.array_equal(got["n"], ref["n"])
            for k in ("mean", "m2", "m3"):
                same_bits_or_nan(got[k], ref[k], "fused %s: %s.%s" % (fmt, t, k))


def fold_records(oracle, state, pixels, values, transform, mm):
    """The definition of statmc_accumulate_records with the oracle: per pixel the records in ascending record index, one sample at
    a time over the pixels that still have one.  values [n_records, C]; records outside the film are skipped.  In place."""
    H, W = state["n"].shape
    live = np.flatnonzero((pixels >= 0) & (pixels < H * W))
    order = live[np.argsort(pixels[live], kind="stable")]
    px = pixels[order]
    rank = np.arange(px.size) - np.searchsorted(px, px, side="left")          # the record's place in its pixel's run
    flat = {k: a.reshape(H * W, -1) if k != "n" else a.reshape(H * W) for k, a in state.items()}
    for s in range(int(rank.max()) + 1 if px.size else 0):
        sel = rank == s
        p = px[sel]
        sub = {k: np.ascontiguousarray(a[p]).reshape((1, p.size) + a.shape[1:]) for k, a in flat.items()}
        oracle.accumulate(sub, np.ascontiguousarray(values[order[sel]], np.float32).reshape(1, 1, p.size, -1), transform, mm)
        for k, a in flat.items():
            a[p] = sub[k].reshape((p.size,) + a.shape[1:])
    return state


def records_case(W, H, c, seed):
    """Run lengths 0 .. 17 per pixel, shuffled, a few records outside the film; the heavy-tailed recipe over the records."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 18, W * H)
    px = np.concatenate([np.repeat(np.arange(W * H, dtype=np.int32), counts), np.array([-1, W * H + 7, -5], np.int32)])
    px = px[rng.permutation(px.size)]
    vals = heavy_tailed_samples(rng, 1, 1, px.size, c).reshape(px.size, c)
    planted = np.flatnonzero(~np.isfinite(vals).all(1) | (vals < 0).any(1))
    assert len(planted) == 2
    px[planted] = np.where((px[planted] < 0) | (px[planted] >= W * H), 3, px[planted])      # (the planted samples belong to live records)
    live = (px >= 0) & (px < W * H)
    return np.bincount(px[live], minlength=W * H), px, vals


def test_records(gpu, oracle):
    """statmc_accumulate_records on 37 x 29, run lengths 0 to 17 from a ragged host-made state: PixelStats<3, 3, true>."""
    W, H = 37, 29
    counts, px, vals = records_case(W, H, 3, seed=61)
    v = device_box_cox(gpu, vals)
    rng = np.random.default_rng(62)
    start = random_start_state(rng, H, W, 3, rng.integers(0, 30, (H, W)))
    st = dev_state(start)
    pre = (torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 3, device=DEV))
    d_vals, d_px = to_dev(vals), to_dev(px)
    gpu.accumulate_records(W, H, [gpu.make_stat_type_records(d_vals, 3, st, True, 3, prepass_into=pre)], d_px)
    got = host(st)
    ref_chain = fold_records(oracle, {k: a.copy() for k, a in start.items()}, px, v, False, 3)
    ref_film = fold_records(oracle, {k: a.copy() for k, a in start.items()}, px, vals, True, 3)
    assert np.array_equal(got["n"], start["n"] + counts.reshape(H, W))
    v_inf = np.zeros((H * W, 3), bool)
    live = (px >= 0) & (px < W * H)
    np.logical_or.at(v_inf, px[live], np.isinf(vals[live]))
    assert_chain(oracle, "records", start, got, ref_chain, ref_film, v_inf.reshape(H, W, 3), 3)
    # the epilogue writes the pixels that received records
    touched = counts.reshape(H, W) > 0
    mc_ref, dc_ref = oracle.prepass(got["n"], got["mean"], got["m2"], got["m3"])
    same_bits_or_nan(pre[0].cpu().numpy()[touched], mc_ref[touched], "records: mean_corr", channels=3)
    same_bits_or_nan(pre[1].cpu().numpy()[touched], dc_ref[touched], "records: disc", channels=3)


def test_records_interleaved_fused_kernel(gpu, oracle):
    """One statmc_accumulate_records_interleaved launch of the shipped five types that takes records_interleaved_fused_kernel."""
    W, H = 37, 29
    kinds = [("radiance", 3, True, 3), ("albedo", 3, False, 1), ("normal", 3, False, 1), ("depth", 1, False, 1), ("id", 1, False, 1)]
    counts, px, vals = records_case(W, H, 3, seed=71)
    rng = np.random.default_rng(72)
    fields = [vals] + [rng.random((px.size, c), dtype=np.float32) for _, c, _, _ in kinds[1:]]
    v = device_box_cox(gpu, vals)
    start = [random_start_state(rng, H, W, c, rng.integers(0, 30, (H, W))) for _, c, _, _ in kinds]
    for s, (_, _, tr, _) in zip(start, kinds):
        if not tr:
            s["film_mean"], s["film_m2"] = s["mean"].copy(), s["m2"].copy()
    sts = [dev_state(s) for s in start]
    rec, layout = gpu.pack_records(px, fields)
    types = [gpu.make_stat_type_record_field(c, sts[i], tr, mm) for i, (_, c, tr, mm) in enumerate(kinds)]
    gpu.accumulate_records_interleaved_path(gpu.RECORDS_PATH_FUSED)
    try:
        d_rec = to_dev(rec)
        gpu.accumulate_records_interleaved(W, H, types, d_rec, layout)
        assert gpu.last_accumulate_records_interleaved_path() == gpu.RECORDS_PATH_FUSED
    finally:
        gpu.accumulate_records_interleaved_path(gpu.RECORDS_PATH_AUTO)
    got = host(sts[0])
    ref_chain = fold_records(oracle, {k: a.copy() for k, a in start[0].items()}, px, v, False, 3)
    ref_film = fold_records(oracle, {k: a.copy() for k, a in start[0].items()}, px, vals, True, 3)
    v_inf = np.zeros((H * W, 3), bool)
    live = (px >= 0) & (px < W * H)
    np.logical_or.at(v_inf, px[live], np.isinf(vals[live]))
    assert_chain(oracle, "interleaved fused", start[0], got, ref_chain, ref_film, v_inf.reshape(H, W, 3), 3)
    for i in range(1, len(kinds)):
        ref = fold_records(oracle, {k: a.copy() for k, a in start[i].items()}, px, fields[i], False, 1)
        g = host(sts[i])
        assert np.array_equal(g["n"], ref["n"])
        same_bits_or_nan(g["mean"], ref["mean"], "interleaved fused: %s.mean" % kinds[i][0])
