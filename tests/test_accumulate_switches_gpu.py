"""Every position of the accumulation's debug switches (include/statmc_debug.h) against the bits of the default position.

The switches choose between kernel instantiations and launch shapes that compute the same thing: the LDS-DMA walk against loads
into registers, the deeper prefetch of the mean-only types, the capped / one-pass / resident grids, the ring's first rows requested
ahead of the state, and, tile-fed, the item order and the grid size.  Each position must leave every image -- the counts and the
pre-pass epilogue's two images included -- bit for bit as the default position leaves it; the default position itself is held
against the oracle the way tests/test_gpu_parity.py does it."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_gpu_parity import DEV, TOL, dev_state, to_dev

pytestmark = pytest.mark.gpu

# (name, channels, transform, max_moment): the five shipped stat types (statmc_amd/film.py: STAT_TYPES)
TYPES = [("radiance", 3, True, 3), ("normal", 3, False, 1), ("albedo", 3, False, 1), ("depth", 1, False, 1), ("materialid", 1, False, 1)]
IMAGES = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
# ring depth 3 and one more; one past twice the prefetch depth of the register walk for U = 3, 6 and 12
BATCHES = (1, 3, 4, 7, 13, 25)
DEFAULT = dict(dma=1, umul=1, grid_mode=-1, resident=0, dma_first=0)
POSITIONS = {
    "dma0": dict(dma=0),
    "umul2-dma0": dict(umul=2, dma=0),
    "grid0": dict(grid_mode=0),
    "grid1": dict(grid_mode=1),
    "resident1": dict(resident=1),
    "resident3": dict(resident=3),
    "dma_first": dict(dma_first=1),
}


def set_film_switches(gpu, dma, umul, grid_mode, resident, dma_first):
    lib = gpu.load()
    gpu.accumulate_dma(dma)
    gpu.check(lib.statmc_debug_accumulate_umul(umul))
    gpu.check(lib.statmc_debug_accumulate_launch(grid_mode, dma_first))
    gpu.accumulate_resident_blocks(resident)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# 260 x 3: 195 groups -- one workgroup of three full waves and one wave of three lanes; 1028 x 2: 514 groups -- a grid-stride walk
# under one resident workgroup; 254 x 7: a pixel count that is no multiple of 4 -- the scalar kernel
@pytest.mark.parametrize("W,H", [(260, 3), (1028, 2), (254, 7)], ids=["260x3", "1028x2", "254x7-scalar"])
def test_film_major_switches_same_bits(gpu, oracle, W, H):
    """All five types in one launch of the per-type kernel (the type-fused walk switched off), the radiance type's epilogue on.
    Two launches per batch length on the same images: the first from a zeroed state (one count per group: the shared-reciprocal
    walk), the second from per-pixel random counts in 0 .. 8 with random moments (the ragged walk)."""
    rng = np.random.default_rng(1000 * W + H)
    gpu.accumulate_fused(-1)
    try:
        for S in BATCHES:
            smps, starts, refs = [], [], []
            for launch in range(2):
                smp, start = {}, {}
                for name, ch, transform, mm in TYPES:
                    v = rng.lognormal(0, 1, size=(S, H, W, ch)).astype(np.float32)
                    v[rng.random(v.shape) < 0.2] = 0.0
                    smp[name] = v
                    st = oracle.new_state(H, W, ch)
                    if launch == 1:
                        n0 = rng.integers(0, 9, size=(H, W)).astype(np.int32)
                        st["n"][...] = n0
                        for k in ("mean", "m2", "m3", "film_mean", "film_m2"):
                            st[k][...] = (rng.random(st[k].shape) * (n0[..., None] > 0)).astype(np.float32)
                        if not transform:
                            st["film_mean"][...] = st["mean"]
                            st["film_m2"][...] = st["m2"]
                    start[name] = st
                ref = {name: {k: v.copy() for k, v in start[name].items()} for name, _, _, _ in TYPES}
                for name, ch, transform, mm in TYPES:
                    oracle.accumulate(ref[name], smp[name], transform, mm)
                smps.append({k: to_dev(v) for k, v in smp.items()})
                starts.append({name: dev_state(st) for name, st in start.items()})
                refs.append(ref)

            def run(position):
                """[launch] -> {type: {image: tensor}}, the radiance type with "mean_corr" and "disc" as well"""
                set_film_switches(gpu, **dict(DEFAULT, **position))
                state = {name: {k: torch.empty_like(v) for k, v in starts[0][name].items()} for name, _, _, _ in TYPES}
                pre = (torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 3, device=DEV))
                out = []
                for launch in range(2):
                    for name in state:
                        for k, v in state[name].items():
                            v.copy_(starts[launch][name][k])
                    sts = [gpu.make_stat_type(smps[launch][name], state[name], transform, mm, prepass_into=pre if name == "radiance" else None)
                           for name, ch, transform, mm in TYPES]
                    gpu.accumulate(W, H, sts)
                    assert gpu.last_accumulate_fused() == 0
                    res = {name: {k: v.clone() for k, v in state[name].items()} for name in state}
                    res["radiance"]["mean_corr"], res["radiance"]["disc"] = pre[0].clone(), pre[1].clone()
                    out.append(res)
                torch.cuda.synchronize()
                return out

            base = run({})
            for pid, position in POSITIONS.items():
                got = run(position)
                for launch in range(2):
                    for name in base[launch]:
                        for k, v in base[launch][name].items():
                            assert same_bits(got[launch][name][k], v), (S, pid, launch, name, k)
            # the default position against the oracle
            for launch in range(2):
                for name, ch, transform, mm in TYPES:
                    what = (S, launch, name)
                    got = {k: v.cpu().numpy() for k, v in base[launch][name].items()}
                    ref = refs[launch][name]
                    assert np.array_equal(got["n"], ref["n"]), what
                    if transform:
                        assert np.array_equal(got["film_mean"], ref["film_mean"]), what
                        assert np.array_equal(got["film_m2"], ref["film_m2"]), what
                        for k in ("mean", "m2", "m3")[:mm]:
                            assert rel_l2(got[k], ref[k]) <= TOL, (what, k)
                        # the epilogue: the oracle's pre-pass of the moments the launch stored
                        mc_ref, d_ref = oracle.prepass(got["n"], got["mean"], got["m2"], got["m3"])
                        assert np.array_equal(got["mean_corr"], mc_ref, equal_nan=True), what
                        assert np.array_equal(got["disc"], d_ref, equal_nan=True), what
                    else:
                        for k in ("mean", "m2", "m3")[:mm]:
                            assert np.array_equal(got[k], ref[k]), (what, k)
    finally:
        set_film_switches(gpu, **DEFAULT)
        gpu.accumulate_fused(0)


@pytest.mark.parametrize("W,H", [(64, 40), (50, 37)], ids=["vector-tiles", "scalar-tiles"])
def test_tile_fed_switches_same_bits(gpu, W, H):
    """The films, tile lists and type set of test_gpu_parity.py::test_accumulate_tiles_matches_oracle (which holds the default
    position against the oracle): prefetch depth 1 | 2 x register loads | LDS-DMA x item order 0 | 1 | 2, and one workgroup per
    CU, against the default (2, LDS-DMA, 2, automatic grid)."""
    rng = np.random.default_rng(W * 1000 + H)
    cfgs = [("radiance", 3, True, 3), ("normal", 3, False, 1), ("depth", 1, False, 2)]
    tiles = [(x, y, min(x + 16, W), min(y + 16, H)) for y in range(0, H, 16) for x in range(0, W, 16)]
    iterations = []
    for it in range(2):
        order = rng.permutation(len(tiles))
        counts = rng.choice([0, 1, 3, 7, 12], size=len(tiles))
        bounds, offsets, off = [], [], 0
        blocks = {name: [] for name, _, _, _ in cfgs}
        for k in order:
            x0, y0, x1, y1 = tiles[k]
            S, npx = int(counts[k]), (x1 - x0) * (y1 - y0)
            bounds.append((x0, y0, x1, y1))
            offsets.append(off)
            size = (S * npx + 3) // 4 * 4                      # blocks start on 4-pixel-sample boundaries
            for name, c, transform, mm in cfgs:
                smp = rng.lognormal(0, 1.5, size=(S, y1 - y0, x1 - x0, c)).astype(np.float32)
                smp[rng.random(smp.shape) < 0.15] = 0.0
                blk = np.zeros(size * c, np.float32)
                blk[:smp.size] = smp.ravel()
                blocks[name].append(blk)
            off += size
        iterations.append(({name: to_dev(np.concatenate(blocks[name])) for name, _, _, _ in cfgs}, to_dev(np.array(bounds, np.int32)),
                           to_dev(np.array(offsets, np.int64)), to_dev(counts[order].astype(np.int32))))
    lib = gpu.load()

    def run(umul, dma, order, wg_per_cu):
        gpu.accumulate_dma(dma)
        gpu.check(lib.statmc_debug_accumulate_tiles_variant(umul, order, wg_per_cu))
        state = {name: {k: torch.zeros(H, W, c, device=DEV) for k in IMAGES[1:]} for name, c, _, _ in cfgs}
        for name in state:
            state[name]["n"] = torch.zeros(H, W, dtype=torch.int32, device=DEV)
        for arenas, bounds, offsets, counts in iterations:
            sts = [gpu.make_stat_type_arena(arenas[name], c, state[name], transform, mm) for name, c, transform, mm in cfgs]
            gpu.accumulate_tiles(W, H, sts, bounds, offsets, counts)
        torch.cuda.synchronize()
        return state

    try:
        base = run(2, 1, 2, 0)
        assert int(base["radiance"]["n"].max()) > 0
        positions = [(umul, dma, order, 0) for umul in (1, 2) for dma in (0, 1) for order in (0, 1, 2)] + [(2, 1, 2, 1)]
        for position in positions:
            if position == (2, 1, 2, 0):
                continue
            got = run(*position)
            for name in base:
                for k, v in base[name].items():
                    assert same_bits(got[name][k], v), (position, name, k)
    finally:
        gpu.accumulate_dma(1)
        gpu.check(lib.statmc_debug_accumulate_tiles_variant(2, 2, 0))
