"""statmc_combine_many on the GPU (include/statmc.h): K independently accumulated parts of every pixel's samples combined in
one call -- bit for bit the left fold of statmc_combine_statistics calls it is defined as, and within the existing bound of
the union of the samples; borrowed counts over several sources, aliased film planes, the pre-pass epilogue, validation,
statmc::device::PixelStats::merge inside a renderer's kernel, FilmStats.combine_ of several films end to end at 1080p and
the offline tool's --combine with three stems."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import FILTER_SD, RADIUS, SD_ALBEDO, SD_NORMAL, rel_l2
from test_combine_gpu import (FIELDS, accumulate_ragged, case_streams, clone, fields_of, new_state, random_state, to_np, union64)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G_DR = [-0.5 / SD_NORMAL ** 2, -0.5 / SD_ALBEDO ** 2]
VARIANTS = [(3, 3, True), (3, 3, False), (3, 2, True), (3, 1, False), (1, 3, True),
            (1, 2, False), (1, 1, True), (1, 1, False), (3, 2, False), (3, 1, True)]
N_SOURCES = [1, 2, 4, 7, 15]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(a, b, what=""):
    """two state dicts (tensors or arrays): every plane and n the same int32 bit patterns"""
    for k in a:
        if a[k] is not None:
            assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


# spec: [(dst state, [source states], channels, max_moment, count_of, prepass_into)]
def run_many(api, W, H, spec):
    es = [api.make_combine_many_entry(d, ss, ch, mm, count_of=c, prepass_into=p) for d, ss, ch, mm, c, p in spec]
    api.combine_many(W, H, es)


def run_fold(api, W, H, spec):
    """the definition: for every source k, one statmc_combine_statistics call with the entries (dst, srcs[k], count_of)"""
    for k in range(len(spec[0][1])):
        api.combine_statistics(W, H, [api.make_combine_entry(d, ss[k], ch, mm, count_of=c, prepass_into=p)
                                      for d, ss, ch, mm, c, p in spec])


def ragged_bounds(rng, count, K):
    """[K + 1, H, W] sample indices: part k of a pixel owns bounds[k] .. bounds[k + 1] - 1.  Uneven cuts; every fifth pixel has
    an empty first part, the next an empty middle part, the next an empty last part, the next all samples in one part."""
    H, W = count.shape
    cuts = np.sort(rng.integers(0, count[None] + 1, size=(K - 1, H, W)), axis=0)
    b = np.concatenate([np.zeros((1, H, W), np.int64), cuts, count[None].astype(np.int64)]).reshape(K + 1, -1)
    cnt = count.reshape(-1)
    idx = np.arange(H * W)
    first, mid, last, one = idx % 5 == 0, idx % 5 == 1, idx % 5 == 2, idx % 5 == 3
    b[1, first] = 0
    m = K // 2
    if m + 1 < K:
        b[m + 1, mid] = b[m, mid]
    else:                                 # two parts: the middle part is the last
        b[m, mid] = cnt[mid]
    b[K - 1, last] = cnt[last]
    j = 1 + (idx % K)                     # the one part that holds everything: part j - 1
    for k in range(1, K):
        b[k, one] = np.where(k < j[one], 0, cnt[one])
    b = np.maximum.accumulate(b, axis=0)
    assert (b[0] == 0).all() and (b[K] == cnt).all() and (np.diff(b, axis=0) >= 0).all()
    return b.reshape(K + 1, H, W).astype(np.int32)


def parts_of(api, smp, bounds, transform, mm):
    return [accumulate_ragged(api, smp, bounds[k], bounds[k + 1] - bounds[k], transform, mm) for k in range(bounds.shape[0] - 1)]


def reshaped(kind, ch, W, H):
    """case_streams' pixels as a W x H image (the statistics are per pixel: where a pixel sits does not matter).  The edge
    stream is 8 x 8 as it comes; 7 x 3 takes seven pixels of an ordinary row, of the constants and of the ragged counts."""
    smp, count, _ = case_streams(kind, ch)
    S = smp.shape[0]
    flat, cnt = smp.reshape(S, -1, ch), count.reshape(-1)
    w0 = count.shape[1]
    if kind == "edge" and (W, H) == (7, 3):
        pix = np.array([r * w0 + x for r in (1, 4, 7) for x in range(7)])
    else:
        pix = np.arange(W * H)
    return np.ascontiguousarray(flat[:, pix].reshape(S, H, W, ch)), np.ascontiguousarray(cnt[pix].reshape(H, W))


# ---------------------------------------------------------------- 1. the left fold, bit for bit
@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("W,H", [(8, 8), (7, 3)])        # 4-pixel groups as dwordx4, and a scalar tail
@pytest.mark.parametrize("ch,mm,transform", VARIANTS)
@pytest.mark.parametrize("n_sources", N_SOURCES)
def test_combine_many_is_the_left_fold_bit_for_bit(gpu, n_sources, ch, mm, transform, W, H, kind):
    api = gpu
    smp, count = reshaped(kind, ch, W, H)
    K = n_sources + 1
    bounds = ragged_bounds(np.random.default_rng(100 * n_sources + W), count, K)
    sizes = np.diff(bounds, axis=0)
    assert (sizes[0] == 0).any() and (sizes[K // 2] == 0).any() and (sizes[K - 1] == 0).any()
    parts = parts_of(api, smp, bounds, transform, mm)
    before = [to_np(p) for p in parts]
    ref = [clone(p) for p in parts]
    run_many(api, W, H, [(parts[0], parts[1:], ch, mm, -1, None)])
    run_fold(api, W, H, [(ref[0], ref[1:], ch, mm, -1, None)])
    torch.cuda.synchronize()
    keys = ["n"] + fields_of(mm, transform)
    same_bits({k: parts[0][k] for k in keys}, ref[0], "dst")
    assert np.array_equal(to_np(parts[0])["n"], count)
    for k in range(1, K):                                   # the sources are read only
        same_bits(before[k], to_np(parts[k]), "source %d" % k)


# ---------------------------------------------------------------- 2. the union of the samples
@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("ch,mm,transform", VARIANTS)
@pytest.mark.parametrize("n_sources", N_SOURCES)
def test_combine_many_matches_the_union(gpu, n_sources, ch, mm, transform, kind):
    """The rule of test_combine_matches_the_union_and_the_formula, unchanged: per field, the combined state is at most twice
    as far from the float64 two-pass moments of all samples as the sequential accumulation is (+ 1e-6); the exact rows of
    the edge stream and the pixels that got samples from one part only are the sequential accumulation's bits."""
    api = gpu
    smp, count, _ = case_streams(kind, ch)
    H, W = count.shape
    K = n_sources + 1
    bounds = ragged_bounds(np.random.default_rng(7 * n_sources + ch), count, K)
    parts = parts_of(api, smp, bounds, transform, mm)
    seq = accumulate_ragged(api, smp, np.zeros_like(count), count, transform, mm)
    run_many(api, W, H, [(parts[0], parts[1:], ch, mm, -1, None)])
    torch.cuda.synchronize()
    got, sq = to_np(parts[0]), to_np(seq)
    assert np.array_equal(got["n"], sq["n"]) and np.array_equal(got["n"], count)
    ref = union64(smp, count, transform)
    fields = fields_of(mm, transform)
    errs = {k: (rel_l2(got[k], ref[k]), rel_l2(sq[k], ref[k])) for k in fields}
    print("K = %d %s: rel L2 to the union (combined, sequential) %s" % (K, kind, {k: "%.3e %.3e" % v for k, v in errs.items()}))
    for k in fields:
        assert errs[k][0] <= 2 * errs[k][1] + 1e-6, (k, errs[k])
    one_part = (np.diff(bounds, axis=0) > 0).sum(axis=0) <= 1
    assert one_part.any()
    for k in fields:
        assert np.array_equal(bits(got[k][one_part]), bits(sq[k][one_part])), k
        if kind == "edge":    # zeros (Box-Cox -2), constants, n = 1
            assert np.array_equal(bits(got[k][[3, 4, 6]]), bits(sq[k][[3, 4, 6]])), k


# ---------------------------------------------------------------- 3. borrowed counts over several sources
def mean_only(rng, H, W, ch):
    return {"mean": torch.from_numpy(rng.normal(0, 1, (H, W, ch)).astype(np.float32)).to(DEV)}


@pytest.mark.parametrize("n_sources", [2, 5])
def test_borrowed_counts_follow_the_owner_source_by_source(gpu, n_sources):
    """film and two G-buffer means weighed with the radiance counts: source k with the owner's running count before source k
    is added.  The same bits wherever the owner stands among the entries, and the bits of the fold of two-part calls."""
    api = gpu
    rng = np.random.default_rng(21)
    H, W = 9, 13
    K = n_sources + 1
    ns = [rng.integers(0, 40, (H, W)).astype(np.int32) for _ in range(K)]
    ns[1][0, :] = 0
    ns[0][1, :] = 0
    rad = [random_state(rng, H, W, 3, True, n) for n in ns]
    film, nrm, dep = ([mean_only(rng, H, W, c) for _ in range(K)] for c in (3, 3, 1))

    def spec_for(owner_at, r, f, g, d):
        borrowers = [(f[0], f[1:], 3, 1), (g[0], g[1:], 3, 1), (d[0], d[1:], 1, 1)]
        spec = [b + (owner_at, None) for b in borrowers]
        spec.insert(owner_at, (r[0], r[1:], 3, 3, -1, None))
        return spec

    outs = []
    for owner_at, runner in ((0, run_many), (2, run_many), (3, run_many), (0, run_fold), (3, run_fold)):
        r, f, g, d = ([clone(s) for s in x] for x in (rad, film, nrm, dep))
        runner(api, W, H, spec_for(owner_at, r, f, g, d))
        torch.cuda.synchronize()
        outs.append((r[0], f[0], g[0], d[0]))
        for x, x0 in ((r, rad), (f, film), (g, nrm), (d, dep)):
            for k in range(1, K):
                same_bits(x[k], x0[k], "source %d" % k)
    assert np.array_equal(outs[0][0]["n"].cpu().numpy(), sum(ns))
    assert not torch.equal(outs[0][1]["mean"], film[0]["mean"])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            same_bits(a, b)


# ---------------------------------------------------------------- 4. aliased film planes
def test_aliased_film_images_are_combined_once(gpu):
    api = gpu
    rng = np.random.default_rng(4)
    H, W, K = 6, 10, 4
    st = [random_state(rng, H, W, 3, False, rng.integers(0, 30, (H, W)).astype(np.int32)) for _ in range(K)]
    for s in st:
        s["m2"].abs_()
    ref = [clone(s) for s in st]
    for s in st + ref:
        s["film_mean"], s["film_m2"] = s["mean"], s["m2"]
    plain = [{k: v for k, v in clone(s).items() if not k.startswith("film")} for s in st]
    run_many(api, W, H, [(st[0], st[1:], 3, 2, -1, None)])
    run_fold(api, W, H, [(ref[0], ref[1:], 3, 2, -1, None)])
    run_many(api, W, H, [(plain[0], plain[1:], 3, 2, -1, None)])
    torch.cuda.synchronize()
    for k in ("n", "mean", "m2"):
        assert np.array_equal(bits(st[0][k]), bits(ref[0][k])), k
        assert np.array_equal(bits(st[0][k]), bits(plain[0][k])), k


# ---------------------------------------------------------------- 5. the pre-pass epilogue
@pytest.mark.parametrize("dof", ["pixel", "welch"])
def test_prepass_epilogue_is_the_prepass_of_the_final_moments(gpu, dof):
    api = gpu
    smp, count, _ = case_streams("edge", 3)
    H, W = count.shape
    bounds = ragged_bounds(np.random.default_rng(9), count, 4)
    parts = parts_of(api, smp, bounds, True, 3)
    mc, dc = torch.full((H, W, 3), 7.0, device=DEV), torch.full((H, W, 3), 7.0, device=DEV)
    try:
        if dof == "welch":
            api.set_filter_spec(dof=api.DOF_WELCH)
        run_many(api, W, H, [(parts[0], parts[1:], 3, 3, -1, (mc, dc))])
        A = parts[0]
        mc2, dc2 = torch.zeros_like(mc), torch.zeros_like(dc)
        args, keep = api.make_filter_args(n=[A["n"]], mean=[A["mean"]], m2=[A["m2"]], m3=[A["m3"]], film=[A["film_mean"]],
                                          mean_corr=[mc2], disc=[dc2], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
        api.prepass(args, 3)
        torch.cuda.synchronize()
    finally:
        api.set_filter_spec()
    assert np.array_equal(A["n"].cpu().numpy(), count)
    assert np.array_equal(bits(mc), bits(mc2))
    assert np.array_equal(bits(dc), bits(dc2))


# ---------------------------------------------------------------- 6. validation, no-ops, the largest call
def test_validation_leaves_dst_untouched(gpu):
    api = gpu
    lib = api.load()
    rng = np.random.default_rng(6)
    H, W = 4, 8
    mk = lambda: random_state(rng, H, W, 3, True, rng.integers(1, 9, (H, W)).astype(np.int32))
    A, B1, B2, F0, F1, F2 = mk(), mk(), mk(), mk(), mk(), mk()
    A0, F00 = to_np(A), to_np(F0)
    film = lambda s: {"mean": s["mean"]}
    M = api.make_combine_many_entry

    def rc(entries, n_sources, n=None):
        arr = (api.CombineManyEntry * max(len(entries), 1))(*entries)
        return lib.statmc_combine_many(W, H, arr, len(entries) if n is None else n, n_sources, None)

    ok = lambda: M(A, [B1, B2], 3, 3)
    bad = []
    bad.append(("too many sources", [M(A, [B1] * 16, 3, 3)], 16))
    bad.append(("negative n_sources", [ok()], -1))
    bad.append(("too many entries", [ok()] * 17, 2))
    e = ok(); e.srcs = None; bad.append(("null srcs", [e], 2))
    e = ok(); e._srcs[1].channels = 1; bad.append(("a part's channels", [e], 2))
    e = ok(); e._srcs[1].max_moment = 2; bad.append(("a part's max_moment", [e], 2))
    e = ok(); e._srcs[1].m3 = None; bad.append(("a part's null m3", [e], 2))
    e = ok(); e._srcs[1].n = None; bad.append(("a part's null n", [e], 2))
    e = ok(); e._srcs[1].m2 = e.dst.m2; bad.append(("dst.m2 is a source's m2", [e], 2))
    e = ok(); e._srcs[1].m2 = e.dst.mean; bad.append(("dst.mean is a source's m2", [e], 2))
    e = ok(); e._srcs[1].n = e.dst.n; bad.append(("dst.n is a source's n", [e], 2))
    e = ok(); e._srcs[0].film_mean = e.dst.film_mean; bad.append(("dst.film_mean is a source's", [e], 2))
    bad.append(("two owners of one count image", [ok(), M(A, [F1, F2], 3, 3)], 2))
    bad.append(("borrow from a borrower", [ok(), M(film(F0), [film(F1), film(F2)], 3, 1, count_of=0),
                                           M(film(B1), [film(F1), film(F2)], 3, 1, count_of=1)], 2))
    bad.append(("count_of out of range", [ok(), M(film(F0), [film(F1), film(F2)], 3, 1, count_of=5)], 2))
    e = M(film(F0), [film(F1), film(F2)], 3, 1, count_of=0); e._srcs[1].n = F2["n"].data_ptr()
    bad.append(("a borrower's part with n", [ok(), e], 2))
    # a valid first entry does not get combined when a later one is refused
    e = M(F0, [F1, F2], 3, 3); e._srcs[1].mean = None
    bad.append(("second entry's null mean", [ok(), e], 2))
    for what, es, k in bad:
        assert rc(es, k) == api.ERR_INVALID, what
        assert lib.statmc_last_error(), what
    assert lib.statmc_combine_many(W, H, None, 1, 1, None) == api.ERR_INVALID
    torch.cuda.synchronize()
    same_bits(A0, to_np(A), "dst after refused calls")
    same_bits(F00, to_np(F0), "dst after refused calls")
    # no-ops
    assert rc([ok()], 0) == api.STATMC_OK and rc([], 3, 0) == api.STATMC_OK and rc([], 0, 0) == api.STATMC_OK
    api.combine_many(W, H, [M(A, [], 3, 3)])
    torch.cuda.synchronize()
    same_bits(A0, to_np(A), "dst after n_sources = 0")
    assert rc([ok()], 2) == api.STATMC_OK
    torch.cuda.synchronize()
    assert np.array_equal(to_np(A)["n"], A0["n"] + to_np(B1)["n"] + to_np(B2)["n"])


@pytest.mark.parametrize("W,H", [(12, 5), (9, 3)])
def test_sixteen_entries_of_fifteen_sources(gpu, W, H):
    """The largest call: an owner with every plane, own-count entries of every shape and borrowers, 16 in all, 15 sources
    each -- more than one launch holds -- equals the fold."""
    api = gpu
    rng = np.random.default_rng(16)
    K = 16
    cnt = lambda: rng.integers(0, 12, (H, W)).astype(np.int32)
    shapes = [(3, 3, True, -1), (3, 1, False, 0), (1, 1, False, 0), (3, 2, True, -1), (1, 3, True, -1), (3, 1, False, 6),
              (1, 2, False, -1), (3, 3, False, -1), (3, 1, True, -1), (1, 1, False, 6), (3, 2, False, -1), (1, 1, True, -1),
              (3, 1, False, 0), (1, 3, False, -1), (3, 3, True, -1), (1, 2, True, -1)]
    spec = []
    for ch, mm, tr, count_of in shapes:
        if count_of < 0:
            st = [random_state(rng, H, W, ch, tr, cnt()) for _ in range(K)]
        else:
            st = [mean_only(rng, H, W, ch) for _ in range(K)]
        spec.append((st[0], st[1:], ch, mm, count_of, None))
    assert len(spec) == 16
    ref = [(clone(d), [clone(s) for s in ss], ch, mm, c, p) for d, ss, ch, mm, c, p in spec]
    run_many(api, W, H, spec)
    run_fold(api, W, H, ref)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(spec, ref)):
        same_bits(a[0], b[0], "entry %d" % i)
        for k in range(K - 1):
            same_bits(a[1][k], b[1][k], "entry %d source %d" % (i, k))


# ---------------------------------------------------------------- 7. merge inside a renderer's kernel
@pytest.fixture(scope="module")
def example(gpu):
    from statmc_amd import api, build
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.fold_arena_slots.argtypes = [C.POINTER(api.StatType), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.POINTER(api.PrepassContext), C.c_void_p]
    return lib


@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("ch,mm,transform", [(3, 3, True), (1, 3, False), (3, 2, True), (1, 2, False), (3, 1, False), (1, 1, True)])
@pytest.mark.parametrize("P", [2, 3, 8])
def test_merge_in_a_kernel_is_combine_many_of_the_slots(gpu, example, P, ch, mm, transform, kind):
    """Every pixel's samples dealt unevenly to P slots (some get none), each slot folded with PixelStats::add and the slots
    merged in slot order inside one kernel: the bits of P states made by statmc_accumulate, combined by statmc_combine_many
    in slot order; store(t, pixel, ctx) writes the pre-pass of those moments."""
    api = gpu
    smp, count, _ = case_streams(kind, ch)
    H, W = count.shape
    bounds = ragged_bounds(np.random.default_rng(30 + P), count, P)
    assert (np.diff(bounds, axis=0) == 0).any()
    arena = torch.from_numpy(smp).to(DEV)
    b_dev = torch.from_numpy(bounds).to(DEV)
    st = new_state(H, W, ch, transform)
    with_pre = mm == 3
    mc, dc = torch.full((H, W, ch), 7.0, device=DEV), torch.full((H, W, ch), 7.0, device=DEV)
    t = api.make_stat_type(arena, st, transform, mm, prepass_into=(mc, dc) if with_pre else None)
    ctx = api.prepass_context()
    api.check(example.fold_arena_slots(C.byref(t), W, H, arena.data_ptr(), b_dev.data_ptr(), P, C.byref(ctx) if with_pre else None,
                                       api.current_stream_handle()))
    parts = parts_of(api, smp, bounds, transform, mm)
    mc2, dc2 = torch.zeros_like(mc), torch.zeros_like(dc)
    run_many(api, W, H, [(parts[0], parts[1:], ch, mm, -1, (mc2, dc2) if with_pre else None)])
    torch.cuda.synchronize()
    keys = ["n"] + fields_of(mm, transform)
    same_bits({k: st[k] for k in keys}, parts[0], "P = %d" % P)
    assert np.array_equal(st["n"].cpu().numpy(), count)
    if with_pre:
        assert np.array_equal(bits(mc), bits(mc2)) and np.array_equal(bits(dc), bits(dc2))
        if ch == 3:
            mc3, dc3 = torch.zeros_like(mc), torch.zeros_like(dc)
            fm = st["film_mean"] if transform else st["mean"]
            args, keep = api.make_filter_args(n=[st["n"]], mean=[st["mean"]], m2=[st["m2"]], m3=[st["m3"]], film=[fm],
                                              mean_corr=[mc3], disc=[dc3], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
            api.prepass(args, 3)
            torch.cuda.synchronize()
            assert np.array_equal(bits(mc), bits(mc3)) and np.array_equal(bits(dc), bits(dc3))


# ---------------------------------------------------------------- 8. FilmStats.combine_ of several films, 1080p
def test_filmstats_combine_many_end_to_end_1080p(gpu, oracle):
    """256 spp as four parts of 64 at 1920 x 1080: combine_([b, c, d]) + the denoise is, bit for bit, three combine_ calls + the
    denoise; and within 1e-5 of the oracle's pre-pass and filter of the combined moments on the strips
    tests/test_gpu_fullsize.py checks, like test_filmstats_combine_end_to_end_1080p for two parts."""
    from statmc_amd import film, synthetic
    W, H = 1920, 1080
    scene = synthetic.Scene(W, H, seed=1, device=DEV)
    many = [film.FilmStats(W, H, DEV, fused_prepass=(k == 0)) for k in range(4)]
    step = [film.FilmStats(W, H, DEV, fused_prepass=(k == 0)) for k in range(4)]
    seq = film.FilmStats(W, H, DEV)
    for k, seed in enumerate((2, 3, 4, 5)):
        smp = scene.samples(64, seed=seed, features=("radiance", "normal", "albedo"))
        for f in (many[k], step[k], seq):
            f.accumulate(smp)
        # the colour image of each part: its own radiance mean
        for f in (many[k], step[k]):
            f.film.copy_(f.state["radiance"]["film_mean"])
        del smp
    seq.film.copy_(seq.state["radiance"]["film_mean"])
    many[0].combine_(many[1:])
    for o in step[1:]:
        step[0].combine_(o)
    assert many[0]._prepass_current is not None
    a, b = many[0], step[0]
    for t in a.types:
        same_bits(a.state[t], b.state[t], t)
        assert torch.equal(a.state[t]["n"], seq.state[t]["n"])
    assert np.array_equal(bits(a.film), bits(b.film))
    assert np.array_equal(bits(a.mean_corr), bits(b.mean_corr)) and np.array_equal(bits(a.disc), bits(b.disc))
    for k in range(1, 4):
        for t in a.types:
            same_bits(many[k].state[t], step[k].state[t], "part %d %s" % (k, t))
    out = a.denoise().clone()
    out_step = b.denoise().clone()
    whole = seq.denoise().clone().cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(out_step))
    rad = {k: v.cpu().numpy() for k, v in a.state["radiance"].items()}
    mc, dc = oracle.prepass(rad["n"], rad["mean"], rad["m2"], rad["m3"])
    gbs = [a.g_buffer("normal").cpu().numpy(), a.g_buffer("albedo").cpu().numpy()]
    got = out.cpu().numpy()
    for roi in ((0, 530, W, 546), (0, 0, 300, 8), (W - 300, H - 8, W, H)):
        x0, y0, x1, y1 = roi
        ref = oracle.filter_image(mc, dc, rad["film_mean"], gbs, G_DR, -0.5 / FILTER_SD ** 2, RADIUS, roi=roi)[y0:y1, x0:x1]
        for c in range(3):
            e = rel_l2(got[y0:y1, x0:x1, c], ref[..., c])
            print("roi %s channel %d: rel L2 to the oracle %.3e" % (roi, c, e))
            assert e <= 1e-5, (roi, c)
    errs = [rel_l2(got[..., c], whole[..., c]) for c in range(3)]
    print("combined 4 x 64 vs sequential 256 spp, whole frame rel L2 per channel: %s" % ["%.3e" % e for e in errs])
    assert max(errs) <= 1e-3


# ---------------------------------------------------------------- 9. the offline tool, three stems
def test_offline_tool_combines_three_stems_like_stem_by_stem(gpu, oracle, tmp_path):
    """--combine b,c --write-combined writes the PFM bytes that combining stem by stem through an intermediate
    --write-combined dump writes (counts stay far below 2^24, so n survives the float PFM), film-f included."""
    from statmc_amd import build, pfm, synthetic
    from statmc_amd.film import STAT_TYPES
    exe = build.build_tools()
    W, H, S = 96, 40, 8
    scene = synthetic.Scene(W, H, seed=5)
    names = ["film", "t0-b0-n", "t0-b0-mean", "t0-b0-m2", "t0-b0-m3", "t1-b0-film-mean", "t2-b0-film-mean"]
    stems = [str(tmp_path / s) for s in "abc"]
    for stem, seed in zip(stems, (6, 7, 8)):
        smp = {k: v.numpy() for k, v in scene.samples(S, seed=seed, features=("radiance", "normal", "albedo")).items()}
        st = {}
        for t in ("radiance", "normal", "albedo"):
            st[t] = oracle.new_state(H, W, 3)
            oracle.accumulate(st[t], smp[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"])
        r = st["radiance"]
        dump = {"film": r["film_mean"], "t0-b0-n": r["n"], "t0-b0-mean": r["mean"], "t0-b0-m2": r["m2"], "t0-b0-m3": r["m3"],
                "t1-b0-film-mean": st["normal"]["mean"], "t2-b0-film-mean": st["albedo"]["mean"]}
        assert sorted(dump) == sorted(names)
        for name, img in dump.items():
            pfm.write_pfm("%s-%d-%s.pfm" % (stem, S, name), img)
    args = ["--filtersd", str(FILTER_SD), "--filterradius", str(RADIUS), "--output", "film-f"]

    def run(stem, spp, combine, out):
        r = subprocess.run([exe, "--stem", stem, "--spp", str(spp), "--combine", combine, "--output-stem", out, "--write-combined"]
                           + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return r.stdout

    one = str(tmp_path / "one")
    assert "groups of 2" in run(stems[0], S, stems[1] + "," + stems[2], one)            # -> one-<3S>-*
    ab = str(tmp_path / "ab")
    run(stems[0], S, stems[1], ab)                                                        # -> ab-<2S>-*
    os.remove("%s-%d-film-f.pfm" % (ab, 2 * S))                                           # a result, not part of the dump
    c2 = str(tmp_path / "c2")                                                             # c's dump under ab's sample count
    for name in names:
        shutil.copy("%s-%d-%s.pfm" % (stems[2], S, name), "%s-%d-%s.pfm" % (c2, 2 * S, name))
    two = str(tmp_path / "two")
    run(ab, 2 * S, c2, two)                                                               # -> two-<4S>-*
    for name in names + ["film-f"]:
        a = open("%s-%d-%s.pfm" % (one, 3 * S, name), "rb").read()
        b = open("%s-%d-%s.pfm" % (two, 4 * S, name), "rb").read()
        assert a == b, name
    assert np.array_equal(pfm.read_pfm("%s-%d-t0-b0-n.pfm" % (one, 3 * S)), np.full((H, W), 3 * S, np.float32))
    assert np.isfinite(pfm.read_pfm("%s-%d-film-f.pfm" % (one, 3 * S))).all()
    # the memory bound only changes the grouping: one stem at a time gives the same bytes
    r = subprocess.run([exe, "--stem", stems[0], "--spp", str(S), "--combine", stems[1] + "," + stems[2], "--output-stem",
                        str(tmp_path / "small"), "--write-combined", "--combine-mem", "0"] + args, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "groups of 1" in r.stdout, r.stderr
    for name in names + ["film-f"]:
        assert open("%s-%d-%s.pfm" % (one, 3 * S, name), "rb").read() == \
            open("%s-%d-%s.pfm" % (str(tmp_path / "small"), 3 * S, name), "rb").read(), name
