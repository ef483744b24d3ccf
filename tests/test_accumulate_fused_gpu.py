"""The accumulation's type-fused walk (accumulate_fused_kernel: one wave folds every stat type of its pixel groups in one pass over
the samples) against the per-type kernel it stands in for: the same samples from the same initial state through both, every
plane of every type compared bit for bit -- and the launch asked whether it really ran fused (a comparison that silently fell
back would prove nothing).  Shapes: the smallest at which each mechanism of the walk can break."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SET9 = ("radiance", "normal", "albedo")
SET11 = ("radiance", "normal", "albedo", "depth", "materialid")
ORDERS = {SET9: ("normal", "radiance", "albedo"), SET11: ("depth", "normal", "materialid", "radiance", "albedo")}
RING = 3          # rows in flight per wave (kAccFusedD); the batch lengths below sit around it


@functools.lru_cache(maxsize=None)
def samples(W, H, S, seed=7):
    """{type: [S, H, W, C]}: positive radiance with exact zeros and a few large values, features in [0, 1).  Computed once per shape."""
    from statmc_amd import synthetic
    g = torch.Generator(device=DEV).manual_seed(seed + 1000 * W + H)
    out = {}
    for t in SET11:
        x = torch.rand(S, H, W, synthetic.CHANNELS[t], device=DEV, generator=g)
        if t == "radiance":
            x = torch.where(x < 0.2, torch.zeros_like(x), x * 3.0)
            x = torch.where(x > 2.99, x * 400.0, x)
        out[t] = x
    return out


def cut(smp, types, a, b):
    return {t: smp[t][a:b].contiguous() for t in types}


def new_film(gpu, W, H, types, epilogue, warm=2):
    """A film that has seen `warm` samples per pixel through the per-type kernel: non-trivial moments, one count everywhere."""
    from statmc_amd import film
    fs = film.FilmStats(W, H, DEV, types=types, fused_prepass=epilogue)
    if warm:
        gpu.accumulate_fused(-1)
        try:
            fs.accumulate(cut(samples(W, H, warm, seed=3), types, 0, warm))
        finally:
            gpu.accumulate_fused(0)
    return fs


def accumulate(gpu, fs, smp, mode, blocks=0):
    """One launch with the switch at `mode`; returns whether it ran the fused walk, and the launch's workgroups."""
    lib = gpu.load()
    gpu.accumulate_fused(mode)
    gpu.accumulate_resident_blocks(blocks)
    try:
        fs.accumulate(smp)
        return gpu.last_accumulate_fused(), lib.statmc_debug_last_accumulate_grid()
    finally:
        gpu.accumulate_fused(0)
        gpu.accumulate_resident_blocks(0)


def assert_same_bits(fa, fb, epilogue):
    torch.cuda.synchronize()
    for t in fa.types:
        for k, v in fa.state[t].items():
            if v is not None:
                assert torch.equal(v.view(torch.int32), fb.state[t][k].view(torch.int32)), (t, k)
    if epilogue:
        assert torch.equal(fa.mean_corr.view(torch.int32), fb.mean_corr.view(torch.int32)), "mean_corr"
        assert torch.equal(fa.disc.view(torch.int32), fb.disc.view(torch.int32)), "disc"


def both_ways(gpu, W, H, types, S, epilogue, prepare=None, blocks=0, expect_fused=1):
    smp = cut(samples(W, H, S), types, 0, S)
    fa, fb = new_film(gpu, W, H, types, epilogue), new_film(gpu, W, H, types, epilogue)
    if prepare is not None:
        prepare(fa)
        prepare(fb)
    fused, grid = accumulate(gpu, fa, smp, 1, blocks)
    plain, _ = accumulate(gpu, fb, smp, -1)
    assert fused == expect_fused and plain == 0, (fused, plain)
    assert_same_bits(fa, fb, epilogue)
    for t in types:
        assert int(fa.state[t]["n"].max()) >= 2 + S
    return grid


@pytest.mark.parametrize("S", [1, RING - 1, RING, RING + 1, RING + 2, 3 * RING])
@pytest.mark.parametrize("types", [SET9, SET11], ids=["9ch", "11ch"])
def test_one_workgroup_of_full_waves(gpu, types, S):
    """256 x 4 pixels: 256 groups, one workgroup, four full waves.  Batches shorter than, equal to, one more than and about three
    times the ring depth; the pre-pass epilogue on and off; the radiance type first in the list and not."""
    for epilogue in (False, True):
        for order in (types, ORDERS[types]):
            assert both_ways(gpu, 256, 4, order, S, epilogue) == 1


def test_partial_wave_beside_idle_waves(gpu):
    """252 x 5 pixels: 315 groups -- the second workgroup holds one wave of 59 lanes and three waves with nothing to do."""
    for epilogue in (False, True):
        assert both_ways(gpu, 252, 5, SET11, 4, epilogue) == 2


def test_grid_stride_walk_starts_clean_on_every_pass(gpu):
    """512 x 6 pixels: 768 groups = three units on ONE workgroup -- the ring and the counted waits start again on each pass."""
    assert both_ways(gpu, 512, 6, SET11, 5, True, blocks=1) == 1
    assert both_ways(gpu, 512, 6, ORDERS[SET9], 5, False, blocks=1) == 1


def test_types_starting_from_different_counts(gpu):
    """The radiance type has seen three samples the features have not: one reciprocal per type instead of one per sample."""
    def radiance_alone(fs):
        gpu.accumulate_fused(-1)
        try:
            fs.accumulate(cut(samples(256, 4, 3, seed=11), ("radiance",), 0, 3))
        finally:
            gpu.accumulate_fused(0)
    for types in (SET11, ORDERS[SET9]):
        both_ways(gpu, 256, 4, types, 4, True, prepare=radiance_alone)


@pytest.mark.parametrize("ragged_type", ["radiance", "albedo", "depth"])
def test_ragged_counts_fall_back_inside_a_fused_launch(gpu, ragged_type):
    """One type's counts differ inside one 4-pixel group of the second wave, in a launch that reports itself fused: the launch
    leaves the per-type kernel's bits in every wave.  (By design that wave folds its groups through accumulate_lane, type after
    type, and the waves beside it stay on the fused walk; both paths give the same bits, so which wave took which is not something
    this test can see -- it asserts the bits and that the launch was the fused kernel.)"""
    def ragged(fs):
        fs.state[ragged_type]["n"][1, 41] += 2       # pixel 297: group 74, the second wave of the workgroup
    both_ways(gpu, 256, 4, SET11, 4, True, prepare=ragged)

    def ragged_rows(fs):                             # the same through the library: a row range that ends inside the film
        gpu.accumulate_fused(-1)
        try:
            fs.accumulate(cut(samples(256, 4, 1, seed=13), SET11, 0, 1), rows=(0, 2))
        finally:
            gpu.accumulate_fused(0)
        fs.state[ragged_type]["n"][2, 7] += 1
    both_ways(gpu, 256, 4, SET11, 4, False, prepare=ragged_rows)


def test_ineligible_launches_keep_the_per_type_kernel(gpu):
    """A film whose pixels are no multiple of four, two batch lengths in one launch, the radiance type alone: fused = 0 with the
    switch at 1, and the bits of the switch at -1."""
    both_ways(gpu, 254, 3, SET11, 4, True, expect_fused=0)
    both_ways(gpu, 256, 4, ("radiance",), 4, True, expect_fused=0)
    # radiance 4 samples, normal 3
    from statmc_amd import film
    W, H = 256, 4
    smp = samples(W, H, 4)
    fa, fb = new_film(gpu, W, H, SET9, False), new_film(gpu, W, H, SET9, False)
    flags = []
    for fs, mode in ((fa, 1), (fb, -1)):
        sts = [gpu.make_stat_type(smp[t][:3 if t == "normal" else 4].contiguous(), fs.state[t], film.STAT_TYPES[t]["transform"],
                                  film.STAT_TYPES[t]["max_moment"]) for t in SET9]
        gpu.accumulate_fused(mode)
        try:
            gpu.accumulate(W, H, sts)
            flags.append(gpu.last_accumulate_fused())
        finally:
            gpu.accumulate_fused(0)
    assert flags == [0, 0]
    assert_same_bits(fa, fb, False)
    assert int(fa.state["normal"]["n"].max()) == 5 and int(fa.state["radiance"]["n"].min()) == 6


def test_two_fused_batches_chain_like_the_per_type_kernel(gpu):
    """4 samples, then 3, both launches fused, against the same chain through the per-type kernel."""
    W, H = 256, 4
    for types in (SET11, SET9):
        smp = samples(W, H, 7)
        fa, fb = new_film(gpu, W, H, types, True), new_film(gpu, W, H, types, True)
        for a, b in ((0, 4), (4, 7)):
            assert accumulate(gpu, fa, cut(smp, types, a, b), 1)[0] == 1
            assert accumulate(gpu, fb, cut(smp, types, a, b), -1)[0] == 0
        assert_same_bits(fa, fb, True)
        assert int(fa.state["radiance"]["n"].min()) == 9 == int(fb.state[types[-1]]["n"].max())


def test_switch_values(gpu):
    lib = gpu.load()
    assert lib.statmc_debug_accumulate_fused(2) == gpu.ERR_INVALID and lib.statmc_debug_accumulate_fused(-2) == gpu.ERR_INVALID
    # never a resident grid: never the fused walk either, whatever the switch says
    smp = cut(samples(256, 4, 4), SET11, 0, 4)
    fs = new_film(gpu, 256, 4, SET11, False)
    assert accumulate(gpu, fs, smp, 1, blocks=-1)[0] == 0
    assert accumulate(gpu, fs, smp, 0)[0] == 0          # by shape: a film this small keeps the large grid


def test_by_shape_from_128_samples_on_a_quarter_hd_film(gpu):
    """The default switch: 960 x 540, the 9-channel set -- 128 samples per launch run the fused walk on one workgroup per compute
    unit, 64 keep the large grid; the same bits as the per-type kernel either way."""
    from statmc_amd import film
    lib = gpu.load()
    W, H, S = 960, 540, 128
    g = torch.Generator(device=DEV).manual_seed(21)
    smp = {t: torch.rand(S, H, W, 3, device=DEV, generator=g) for t in SET9}
    fa, fb = film.FilmStats(W, H, DEV, types=SET9, fused_prepass=True), film.FilmStats(W, H, DEV, types=SET9, fused_prepass=True)
    for batch in (smp, cut(smp, SET9, 0, 64)):
        fused, grid = accumulate(gpu, fa, batch, 0)
        long_batch = batch is smp
        assert fused == (1 if long_batch else 0), fused
        assert (grid == lib.statmc_device_cus()) == long_batch, grid
        assert accumulate(gpu, fb, batch, -1)[0] == 0
    assert_same_bits(fa, fb, True)
    del smp
