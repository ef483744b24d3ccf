"""include/statmc_device_api.hpp on the GPU: a renderer's own kernel folding samples through statmc::device::PixelStats
(tools/bin/libstatmc_device_example.so, built with hipcc's default floating-point flags) leaves the bits statmc_accumulate
leaves, its pre-pass store writes the bits of statmc_prepass, and a film filled that way denoises to the same bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden")
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
FIVE = ("radiance", "normal", "albedo", "depth", "materialid")   # gen_arena / gen_fold order


@pytest.fixture(scope="module")
def example(gpu):
    from statmc_amd import api, build
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.fold_arena.argtypes = [C.POINTER(api.StatType), C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(api.PrepassContext), C.c_void_p]
    lib.gen_arena.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_void_p]
    lib.gen_fold.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(api.StatType), C.POINTER(api.PrepassContext),
                             C.c_void_p]
    return lib


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_state(a, b, fields=FIELDS):
    for k in fields:
        if a.get(k) is not None:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


def fold(api, lib, W, H, state, samples, transform, max_moment, ctx=None, prepass_into=None):
    t = api.make_stat_type(samples, state, transform, max_moment, prepass_into=prepass_into)
    rc = lib.fold_arena(C.byref(t), W, H, samples.data_ptr(), samples.shape[0], C.byref(ctx) if ctx is not None else None,
                        api.current_stream_handle())
    api.check(rc)


def arena(rng, S, H, W, c, edge=None, s0=0):
    """log-normal samples with 20 % zeros; the top-left 8 x 8 pixels carry samples s0 .. s0 + S - 1 of the edge-case fixture"""
    import torch
    a = np.exp(rng.normal(0.0, 1.0, (S, H, W, c))).astype(np.float32)
    a *= rng.random((S, H, W, 1)) >= 0.2
    if edge is not None:
        a[:, :8, :8, :] = edge[s0:s0 + S, :, :, :c]
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


VARIANTS = [(c, t, m) for c in (1, 3) for t in (0, 1) for m in (1, 2, 3)]


@pytest.mark.parametrize("size", [(61, 37), (64, 36)])       # odd: the library's per-pixel path; aligned: its vector path
@pytest.mark.parametrize("c,t,m", VARIANTS)
def test_fold_arena_is_statmc_accumulate(gpu, example, size, c, t, m):
    import torch
    from statmc_amd import film
    api = gpu
    W, H = size
    edge = np.load(os.path.join(GDIR, "accumulate_edge_cases.npz"))["samples"]   # 24 samples of 8 x 8 pixels
    rng = np.random.default_rng(100 * c + 10 * t + m)
    A = film.new_state(H, W, c, torch.device("cuda:0"), transform=True)
    B = film.new_state(H, W, c, torch.device("cuda:0"), transform=True)
    s0 = 0
    for S in (10, 14):      # the second batch starts from n0 = 10
        smp = arena(rng, S, H, W, c, edge, s0)
        api.accumulate(W, H, [api.make_stat_type(smp, A, t, m)])
        fold(api, example, W, H, B, smp, t, m)
        s0 += S
    torch.cuda.synchronize()
    assert int(B["n"].min()) == int(B["n"].max()) == 24
    same_state(A, B, ("n", "mean") + (("m2",) if m >= 2 else ()) + (("m3",) if m >= 3 else ()) + (("film_mean", "film_m2") if t else ()))


def prepass_of(api, st, c):
    import torch
    mc, dc = torch.zeros_like(st["mean"]), torch.zeros_like(st["mean"])
    args, keep = api.make_filter_args(n=[st["n"]], mean=[st["mean"]], m2=[st["m2"]], m3=[st["m3"]], film=[st["mean"]],
                                      mean_corr=[mc], disc=[dc], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
    api.prepass(args, c)
    return mc, dc


def seeded_state(rng, H, W, c):
    """A state whose pixels hold n0 in {0, 1, 3, 5000}: after one more sample n = 1 (small n), 2, 4 and > 4096 (the last table
    entry); some m2 = 0 (the pre-pass's s2sum > 0 test)."""
    import torch
    n0 = rng.choice(np.array([0, 1, 3, 5000], np.int32), size=(H, W))
    mean = rng.normal(0.5, 0.3, (H, W, c)).astype(np.float32)
    m2 = np.abs(rng.normal(0.0, 1.0, (H, W, c))).astype(np.float32) * (n0[..., None] > 0)
    m3 = rng.normal(0.0, 1.0, (H, W, c)).astype(np.float32) * (n0[..., None] > 0)
    st = {"n": n0, "mean": mean, "m2": m2, "m3": m3, "film_mean": mean.copy(), "film_m2": m2.copy()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def check_store_with_prepass(api, lib, rng, W=37, H=21):
    import torch
    ctx = api.prepass_context()
    for c, t in ((3, 1), (1, 0)):
        A = seeded_state(rng, H, W, c)
        smp = arena(rng, 1, H, W, c)
        zero = rng.random((H, W)) < 0.2                     # sample == mean: d = 0, m2 stays 0 where it was
        if not t:
            smp[0][torch.from_numpy(zero).cuda()] = A["mean"][torch.from_numpy(zero).cuda()]
        mc = torch.full_like(A["mean"], 7.0)
        dc = torch.full_like(A["mean"], 7.0)
        fold(api, lib, W, H, A, smp, t, 3, ctx=ctx, prepass_into=(mc, dc))
        mc2, dc2 = prepass_of(api, A, c)
        torch.cuda.synchronize()
        assert (A["n"] == 1).any() and (A["n"] > 4096).any()
        assert np.array_equal(bits(mc), bits(mc2)), (c, t)
        assert np.array_equal(bits(dc), bits(dc2)), (c, t)


@pytest.mark.parametrize("significance", [0, 1, 2])
@pytest.mark.parametrize("dof", ["pixel", "welch"])
@pytest.mark.parametrize("small_n", ["accept", "exclude"])
def test_store_with_prepass_is_statmc_prepass(gpu, example, significance, dof, small_n):
    api = gpu
    lib = api.load()
    try:
        api.set_filter_spec(dof=api.DOF_WELCH if dof == "welch" else api.DOF_PIXEL, small_n=1 if small_n == "exclude" else 0)
        api.check(lib.statmc_set_significance(significance))
        ctx = api.prepass_context()
        assert ctx.flags == (1 if dof == "welch" else 0) | (2 if small_n == "exclude" else 0)
        check_store_with_prepass(api, example, np.random.default_rng(significance * 4 + (dof == "welch") * 2 + (small_n == "exclude")))
    finally:
        api.set_filter_spec()


def test_store_with_prepass_reads_replaced_quantiles(gpu, example):
    """statmc_set_t_quantiles rewrites the table in place: the context queried before still points at it."""
    api = gpu
    lib = api.load()
    api.set_filter_spec()
    table = api.get_significance() + 3 * api.get_filter_spec().sides   # the table the pre-pass indexes
    ctx_before = api.prepass_context()
    q = (C.c_float * 100)(*np.linspace(9.0, 2.0, 100).astype(np.float32))
    try:
        api.check(lib.statmc_set_t_quantiles(table, q, 100))
        assert api.prepass_context().t_table == ctx_before.t_table
        check_store_with_prepass(api, example, np.random.default_rng(99))
    finally:
        api.check(lib.statmc_set_t_quantiles(table, None, 0))


def five_types(api, fs, S, prepass=False):
    import torch
    from statmc_amd.film import STAT_TYPES
    arr = (api.StatType * 5)()
    for k, name in enumerate(FIVE):
        cfg = STAT_TYPES[name]
        dummy = torch.empty(S, fs.height, fs.width, cfg["channels"], device=fs.device)
        arr[k] = api.make_stat_type(dummy, fs.state[name], cfg["transform"], cfg["max_moment"],
                                    prepass_into=(fs.mean_corr, fs.disc) if (prepass and name == "radiance") else None)
    return arr


def test_gen_fold_is_gen_arena_plus_statmc_accumulate(gpu, example):
    import torch
    from statmc_amd import film
    api = gpu
    W, H, dev = 256, 128, torch.device("cuda:0")
    A = film.FilmStats(W, H, dev, types=FIVE)
    B = film.FilmStats(W, H, dev, types=FIVE)
    st = api.current_stream_handle()
    s0 = 0
    for S in (32, 32):
        arenas = {name: torch.empty(S, H, W, film.STAT_TYPES[name]["channels"], device=dev) for name in FIVE}
        ptrs = (C.c_void_p * 5)(*[arenas[name].data_ptr() for name in FIVE])
        api.check(example.gen_arena(7, W, H, s0, S, ptrs, st))
        A.accumulate(arenas)
        api.check(example.gen_fold(7, W, H, s0, S, five_types(api, B, S), None, st))
        s0 += S
    torch.cuda.synchronize()
    rad = A.state["radiance"]
    assert int(rad["n"].min()) == 64 and float(rad["mean"].std()) > 0
    assert 0.0 <= float(A.state["albedo"]["mean"].min()) and float(A.state["albedo"]["mean"].max()) <= 1.0
    for name in FIVE:
        same_state(A.state[name], B.state[name])
    fa, fb = A.denoise(), B.denoise()
    torch.cuda.synchronize()
    assert np.array_equal(bits(fa), bits(fb))
    assert np.isfinite(fa.cpu().numpy()).all()


def test_gen_fold_store_with_prepass(gpu, example):
    """gen_fold's radiance pre-pass store against statmc_prepass of the moments it leaves."""
    import torch
    from statmc_amd import film
    api = gpu
    W, H, dev = 64, 32, torch.device("cuda:0")
    B = film.FilmStats(W, H, dev, types=FIVE)
    api.set_filter_spec()
    api.check(example.gen_fold(3, W, H, 0, 16, five_types(api, B, 16, prepass=True), C.byref(api.prepass_context()),
                               api.current_stream_handle()))
    mc2, dc2 = prepass_of(api, B.state["radiance"], 3)
    torch.cuda.synchronize()
    assert np.array_equal(bits(B.mean_corr), bits(mc2))
    assert np.array_equal(bits(B.disc), bits(dc2))


def test_estimator_device_statistics_equals_merge_tiles(gpu):
    """C++ host: an Estimator filled through DeviceStatistics + the fused kernel denoises to the bits of one filled through
    Merge*Tile flushes (tests/cpp/test_device_accumulate.cpp)."""
    from statmc_amd import build
    build.build_tools()
    for w, h in ((61, 37), (96, 64)):
        out = subprocess.run([build.DEVICE_ACC_BIN, str(w), str(h)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "device accumulate ok" in out.stdout
