"""statmc::device::merge_lanes / merge_waves on the GPU (include/statmc_device_api.hpp), through the example library's
fold_arena_lanes / fold_arena_waves / fold_arena_lanes_waves / gen_fold_lanes: the states the lanes of a wave or the waves of
a workgroup hold are merged in the header's tree order -- bit for bit the slots' states (statmc_accumulate) combined by
two-part statmc_combine_statistics calls in that order, not statmc_combine_many's left fold -- over launches too, and within
the project's bound of the union of the samples."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_combine_gpu import accumulate_ragged, case_streams, clone, fields_of, new_state, to_np, union64
from test_combine_many_gpu import VARIANTS, bits, parts_of, ragged_bounds, reshaped, run_many, same_bits
from test_device_reduce_cpu import VARIANTS as CPU_VARIANTS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIX = [(3, 3, True), (1, 3, False), (3, 2, True), (1, 2, False), (3, 1, False), (1, 1, True)]   # ch, max_moment, transform
LANES = [2, 4, 8, 16, 32, 64]
WAVES = [2, 4, 8, 16]
FIVE = ("radiance", "normal", "albedo", "depth", "materialid")   # gen_arena / gen_fold order


@pytest.fixture(scope="module")
def example(gpu):
    from statmc_amd import api, build
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    fold = [C.POINTER(api.StatType), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(api.PrepassContext), C.c_void_p]
    lib.fold_arena_lanes.argtypes = fold
    lib.fold_arena_waves.argtypes = fold
    lib.fold_arena_lanes_waves.argtypes = fold[:6] + [C.c_int] + fold[6:]
    lib.gen_arena.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    gen = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(api.StatType), C.POINTER(api.PrepassContext), C.c_void_p]
    lib.gen_fold.argtypes = gen
    lib.gen_fold_lanes.argtypes = gen[:5] + [C.c_int] + gen[5:]
    return lib


def tree(api, W, H, parts, ch, mm, prepass_into=None):
    """The definition: for stride = 1, 2, 4, ...: part j + stride into part j for every j % (2 * stride) == 0, each by one
    two-part statmc_combine_statistics call; the last call (into part 0) writes the pre-pass.  The result is parts[0]."""
    K, stride = len(parts), 1
    assert K & (K - 1) == 0
    while stride < K:
        for j in range(0, K, 2 * stride):
            pre = prepass_into if 2 * stride == K else None
            api.combine_statistics(W, H, [api.make_combine_entry(parts[j], parts[j + stride], ch, mm, prepass_into=pre)])
        stride *= 2
    return parts[0]


def launch(api, example, how, W, H, st, arena, bounds, ch, mm, transform, with_pre):
    """fold_arena_lanes (how = ("lanes", G)), fold_arena_waves (("waves", NW)) or fold_arena_lanes_waves (("both", G, NW)) into
    the state st; returns (mean_corr, discriminator)"""
    mc, dc = torch.full((H, W, ch), 7.0, device=DEV), torch.full((H, W, ch), 7.0, device=DEV)
    t = api.make_stat_type(arena, st, transform, mm, prepass_into=(mc, dc) if with_pre else None)
    ctx = api.prepass_context()
    fn = {"lanes": example.fold_arena_lanes, "waves": example.fold_arena_waves, "both": example.fold_arena_lanes_waves}[how[0]]
    b_dev = torch.from_numpy(bounds).to(DEV)
    api.check(fn(C.byref(t), W, H, arena.data_ptr(), b_dev.data_ptr(), *how[1:], C.byref(ctx) if with_pre else None,
                 api.current_stream_handle()))
    torch.cuda.synchronize()
    return mc, dc


def check_tree_bits(api, example, how, K, ch, mm, transform, W, H, kind):
    smp, count = reshaped(kind, ch, W, H)
    bounds = ragged_bounds(np.random.default_rng(50 + K + W), count, K)
    sizes = np.diff(bounds, axis=0)
    assert (sizes[0] == 0).any() and (sizes[K // 2] == 0).any() and (sizes[K - 1] == 0).any()
    assert ((sizes > 0).sum(axis=0) <= 1).any()
    arena = torch.from_numpy(smp).to(DEV)
    st = new_state(H, W, ch, transform)
    with_pre = mm == 3
    mc, dc = launch(api, example, how, W, H, st, arena, bounds, ch, mm, transform, with_pre)
    parts = parts_of(api, smp, bounds, transform, mm)
    mc2, dc2 = torch.zeros_like(mc), torch.zeros_like(dc)
    ref = tree(api, W, H, parts, ch, mm, (mc2, dc2) if with_pre else None)
    torch.cuda.synchronize()
    keys = ["n"] + fields_of(mm, transform)
    same_bits({k: st[k] for k in keys}, ref, "%s K = %d" % (how[0], K))        # every pixel, every plane
    assert np.array_equal(st["n"].cpu().numpy(), count)
    if with_pre:
        assert np.array_equal(bits(mc), bits(mc2)) and np.array_equal(bits(dc), bits(dc2))
        # ... which are the bits of statmc_prepass on the stored moments (one- and three-channel types alike)
        mc3, dc3 = torch.zeros_like(mc), torch.zeros_like(dc)
        fm = st["film_mean"] if transform else st["mean"]
        args, keep = api.make_filter_args(n=[st["n"]], mean=[st["mean"]], m2=[st["m2"]], m3=[st["m3"]], film=[fm],
                                          mean_corr=[mc3], disc=[dc3], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
        api.prepass(args, ch)
        torch.cuda.synchronize()
        assert np.array_equal(bits(mc), bits(mc3)) and np.array_equal(bits(dc), bits(dc3))


def test_the_cpu_file_compiles_the_variant_list_of_combine_many():
    """tests/test_device_reduce_cpu.py cannot import test_combine_many_gpu (torch, a device): its copy of VARIANTS is checked here"""
    assert CPU_VARIANTS == VARIANTS


# ---------------------------------------------------------------- 1. the tree, bit for bit: the lanes of a wave
@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("W,H", [(8, 8), (7, 3)])     # 7 x 3: a partial last wave for every G < 64, a partial last workgroup for all
@pytest.mark.parametrize("ch,mm,transform", SIX)
@pytest.mark.parametrize("G", LANES)
def test_merge_lanes_is_the_tree_of_two_part_combines(gpu, example, G, ch, mm, transform, W, H, kind):
    check_tree_bits(gpu, example, ("lanes", G), G, ch, mm, transform, W, H, kind)


# ---------------------------------------------------------------- 2. ... the waves of a workgroup, and both
@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("W,H", [(8, 8), (7, 3)])
@pytest.mark.parametrize("ch,mm,transform", SIX)
@pytest.mark.parametrize("NW", WAVES)
def test_merge_waves_is_the_tree_of_two_part_combines(gpu, example, NW, ch, mm, transform, W, H, kind):
    check_tree_bits(gpu, example, ("waves", NW), NW, ch, mm, transform, W, H, kind)


@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("W,H", [(8, 8), (7, 3)])
def test_lanes_then_waves_is_one_tree_over_all_slots(gpu, example, W, H, kind):
    """merge_lanes<4> and then merge_waves<4>: the 16-slot tree with slot index w * 4 + j"""
    check_tree_bits(gpu, example, ("both", 4, 4), 16, 3, 3, True, W, H, kind)
    api = gpu
    t = api.make_stat_type(torch.zeros(1, H, W, 3, device=DEV), new_state(H, W, 3, True), True, 3)
    b = torch.zeros(17, H, W, dtype=torch.int32, device=DEV)
    assert example.fold_arena_lanes_waves(C.byref(t), W, H, b.data_ptr(), b.data_ptr(), 8, 4, None, None) == api.ERR_INVALID


# ---------------------------------------------------------------- 3. not the left fold by accident
def test_the_tree_is_not_the_left_fold_and_keeps_the_exact_cases(gpu, example):
    api = gpu
    G, ch, mm, transform = 8, 3, 3, True
    for kind in ("scene", "edge"):
        smp, count, _ = case_streams(kind, ch)
        H, W = count.shape
        bounds = ragged_bounds(np.random.default_rng(58), count, G)
        st = new_state(H, W, ch, transform)
        launch(api, example, ("lanes", G), W, H, st, torch.from_numpy(smp).to(DEV), bounds, ch, mm, transform, False)
        got = to_np(st)
        sq = to_np(accumulate_ragged(api, smp, np.zeros_like(count), count, transform, mm))
        fields = fields_of(mm, transform)
        if kind == "scene":
            parts = parts_of(api, smp, bounds, transform, mm)
            run_many(api, W, H, [(parts[0], parts[1:], ch, mm, -1, None)])
            torch.cuda.synchronize()
            fold = to_np(parts[0])
            differ = {k: float((bits(got[k]) != bits(fold[k])).mean()) for k in fields}
            print("share of elements whose bits differ between the tree and the left fold, G = 8: %s" % differ)
            assert np.array_equal(got["n"], fold["n"])
            assert any(v > 0 for v in differ.values()), differ
        one_slot = (np.diff(bounds, axis=0) > 0).sum(axis=0) <= 1
        assert one_slot.any()
        for k in fields:
            assert np.array_equal(bits(got[k][one_slot]), bits(sq[k][one_slot])), (kind, k)
            if kind == "edge":    # zeros (Box-Cox -2), constants, n = 1
                assert np.array_equal(bits(got[k][[3, 4, 6]]), bits(sq[k][[3, 4, 6]])), k


# ---------------------------------------------------------------- 4. accumulating over launches
def accumulate_more(api, st, samples, first, count, transform, max_moment):
    """accumulate_ragged, but into the pixels' states in st (a copy is returned): samples[first[p] : first[p] + count[p], p]"""
    S, H, W, Ch = samples.shape
    st = clone(st)
    flat_first, flat_count = first.reshape(-1), count.reshape(-1)
    smp = samples.reshape(S, H * W, Ch)
    for c in sorted(set(int(v) for v in flat_count if v > 0)):
        pix = np.nonzero(flat_count == c)[0]
        idx = flat_first[pix][None, :] + np.arange(c)[:, None]
        part = np.ascontiguousarray(smp[idx, pix[None, :]])[:, None]
        ys, xs = torch.from_numpy(pix // W).to(DEV), torch.from_numpy(pix % W).to(DEV)
        sub = {k: (v[ys, xs][None].contiguous() if v is not None else None) for k, v in st.items()}
        api.accumulate(len(pix), 1, [api.make_stat_type(torch.from_numpy(part).to(DEV), sub, transform, max_moment)])
        for k, v in sub.items():
            if v is not None:
                st[k][ys, xs] = v[0]
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("G", [4, 64])
def test_two_launches_continue_from_the_stored_state(gpu, example, G, kind):
    api = gpu
    ch, mm, transform = 3, 3, True
    smp, count, _ = case_streams(kind, ch)
    H, W = count.shape
    half = (count // 2).astype(np.int32)
    b1 = ragged_bounds(np.random.default_rng(41), half, G)
    b2 = (half[None] + ragged_bounds(np.random.default_rng(42), count - half, G)).astype(np.int32)
    arena = torch.from_numpy(smp).to(DEV)
    st = new_state(H, W, ch, transform)
    launch(api, example, ("lanes", G), W, H, st, arena, b1, ch, mm, transform, False)
    first = clone(st)
    mc, dc = launch(api, example, ("lanes", G), W, H, st, arena, b2, ch, mm, transform, True)
    ref1 = tree(api, W, H, parts_of(api, smp, b1, transform, mm), ch, mm)
    torch.cuda.synchronize()
    keys = ["n"] + fields_of(mm, transform)
    same_bits({k: first[k] for k in keys}, ref1, "first launch")
    parts = parts_of(api, smp, b2, transform, mm)
    parts[0] = accumulate_more(api, ref1, smp, b2[0], b2[1] - b2[0], transform, mm)    # slot 0 starts from the stored state
    mc2, dc2 = torch.zeros_like(mc), torch.zeros_like(dc)
    ref = tree(api, W, H, parts, ch, mm, (mc2, dc2))
    torch.cuda.synchronize()
    same_bits({k: st[k] for k in keys}, ref, "second launch")
    assert np.array_equal(st["n"].cpu().numpy(), count)
    assert np.array_equal(bits(mc), bits(mc2)) and np.array_equal(bits(dc), bits(dc2))


# ---------------------------------------------------------------- 5. the union of the samples
def check_union_rule(got, sq, ref, fields, what):
    """The project's rule (test_combine_many_matches_the_union): per field, at most twice as far (relative L2) from the float64
    two-pass moments of all samples as the sequential accumulation is, + 1e-6."""
    errs = {k: (rel_l2(got[k], ref[k]), rel_l2(sq[k], ref[k])) for k in fields}
    print("%s: rel L2 to the union (merged, sequential) %s" % (what, {k: "%.3e %.3e" % v for k, v in errs.items()}))
    for k in fields:
        assert errs[k][0] <= 2 * errs[k][1] + 1e-6, (what, k, errs[k])


@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("ch,mm,transform", SIX)
@pytest.mark.parametrize("how,K", [(("lanes", G), G) for G in LANES] + [(("waves", NW), NW) for NW in WAVES] + [(("both", 4, 4), 16)])
def test_the_merged_state_matches_the_union(gpu, example, how, K, ch, mm, transform, kind):
    api = gpu
    smp, count, _ = case_streams(kind, ch)
    H, W = count.shape
    bounds = ragged_bounds(np.random.default_rng(7 * K + ch), count, K)
    st = new_state(H, W, ch, transform)
    launch(api, example, how, W, H, st, torch.from_numpy(smp).to(DEV), bounds, ch, mm, transform, False)
    got = to_np(st)
    sq = to_np(accumulate_ragged(api, smp, np.zeros_like(count), count, transform, mm))
    assert np.array_equal(got["n"], count)
    check_union_rule(got, sq, union64(smp, count, transform), fields_of(mm, transform), "%s %s" % (how, kind))


# ---------------------------------------------------------------- 6. the generator with 16 lanes per pixel
def test_gen_fold_lanes_matches_the_union_like_gen_fold(gpu, example):
    from statmc_amd import film
    api = gpu
    W, H, S, G, seed = 64, 48, 40, 16, 5
    stream = api.current_stream_handle()
    arenas = {name: torch.empty(S, H, W, film.STAT_TYPES[name]["channels"], device=DEV) for name in FIVE}
    api.check(example.gen_arena(seed, W, H, 0, S, (C.c_void_p * 5)(*[arenas[name].data_ptr() for name in FIVE]), stream))

    def five(fs):
        arr = (api.StatType * 5)()
        for k, name in enumerate(FIVE):
            cfg = film.STAT_TYPES[name]
            arr[k] = api.make_stat_type(arenas[name], fs.state[name], cfg["transform"], cfg["max_moment"])
        return arr

    lanes, seq = film.FilmStats(W, H, DEV, types=FIVE), film.FilmStats(W, H, DEV, types=FIVE)
    api.check(example.gen_fold_lanes(seed, W, H, 0, S, G, five(lanes), None, stream))
    api.check(example.gen_fold(seed, W, H, 0, S, five(seq), None, stream))
    torch.cuda.synchronize()
    assert example.gen_fold_lanes(seed, W, H, 0, S, 3, five(lanes), None, stream) == api.ERR_INVALID
    count = np.full((H, W), S, np.int32)
    for name in FIVE:
        cfg = film.STAT_TYPES[name]
        got, sq = to_np(lanes.state[name]), to_np(seq.state[name])
        assert np.array_equal(got["n"], count) and np.array_equal(sq["n"], count), name
        ref = union64(arenas[name].cpu().numpy(), count, cfg["transform"])
        check_union_rule(got, sq, ref, fields_of(cfg["max_moment"], cfg["transform"]), name)

