"""statmc_pool_statistics on the GPU (include/statmc.h): the statistics of k x k blocks of fine pixels pooled into one coarse pixel
-- bit for bit the Morton-ordered tree of two-part statmc_combine_statistics calls it is defined as; its exact cases; the
composition pool_a(pool_b) == pool_ab; borrowed counts; the pre-pass epilogue; several entries in one call; the union of the
samples; a stream row; and the host layers (FilmStats.pooled, Estimator::PoolStatistics, statmc_denoise --pool)."""
import subprocess

import numpy as np
import pytest
import torch

from conftest import FILTER_SD, RADIUS, SD_ALBEDO, SD_NORMAL
from test_combine_gpu import accumulate_ragged, case_streams, clone, fields_of, new_state, random_state, to_np, union64
from test_combine_many_gpu import bits, reshaped, same_bits
from test_device_reduce_gpu import SIX, check_union_rule, tree
from test_pool_cpu import KS, coarse, morton
from test_stream_contract_gpu import Case, assert_same_bits, run_gated, run_on_null_stream, side  # noqa: F401  (side: a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 64                   # floats behind every dst plane
SENTINEL = -7.0


# ---------------------------------------------------------------- films and states
def film_stream(kind, ch, W, H):
    """case_streams' pixels as a W x H film (the statistics are per pixel: where a pixel sits does not matter); a film with more
    pixels than the stream has takes them round again"""
    if W * H <= 64:
        return reshaped(kind, ch, W, H)
    smp, count, _ = case_streams(kind, ch)
    S = smp.shape[0]
    pix = np.arange(W * H) % count.size
    return np.ascontiguousarray(smp.reshape(S, -1, ch)[:, pix].reshape(S, H, W, ch)), np.ascontiguousarray(count.reshape(-1)[pix].reshape(H, W))


def planted_counts(rng, avail, k):
    """Per-pixel counts in [0, avail], ragged, with the exact cases planted at two levels of the tree.  2 x 2 sub-blocks (every
    film has several): every fifth without a sample, the next with one live pixel that is not its slot 0, the next with slot 0
    empty and the others live.  k x k blocks, where the film has at least four: the same three, block by block.  Returns
    (counts, cases): cases[name] = list of (X, Y) blocks of size k planted that way."""
    H, W = avail.shape
    cnt = rng.integers(0, avail + 1).astype(np.int32)
    cases = {"empty": [], "one_live_not_slot0": [], "slot0_empty": []}

    def plant(size, x0, y0, what):
        ys, xs = slice(y0, min(y0 + size, H)), slice(x0, min(x0 + size, W))
        inside = [(x, y) for y in range(ys.start, ys.stop) for x in range(xs.start, xs.stop)]
        if what == "empty":
            cnt[ys, xs] = 0
        elif what == "one_live_not_slot0":
            if len(inside) < 2:
                return False
            cnt[ys, xs] = 0
            x, y = inside[-1]
            cnt[y, x] = max(int(avail[y, x]), 1) if avail[y, x] > 0 else 0
            if cnt[y, x] == 0:
                return False
        else:
            if len(inside) < 2:
                return False
            cnt[ys, xs] = np.maximum(avail[ys, xs], 0)
            cnt[y0, x0] = 0
            if cnt[ys, xs].sum() == 0:
                return False
        return True

    names = ["empty", "one_live_not_slot0", "slot0_empty"]
    for i, (y0, x0) in enumerate((y, x) for y in range(0, H, 2) for x in range(0, W, 2)):
        if i % 5 < 3:
            plant(2, x0, y0, names[i % 5])
    Wc, Hc = coarse(W, k), coarse(H, k)
    if Wc * Hc >= 4:
        for i, (Y, X) in enumerate((Y, X) for Y in range(Hc) for X in range(Wc)):
            if i % 4 < 3 and plant(k, X * k, Y * k, names[i % 4]):
                cases[names[i % 4]].append((X, Y))
        assert all(cases.values()), cases
    return cnt, cases


def add_payload(rng, st, cnt):
    """values in the pixels without a sample: which empty slot's bits survive a merge is part of the definition"""
    empty = torch.from_numpy(cnt == 0).to(DEV)
    for key, v in st.items():
        if key != "n" and v is not None:
            v[empty] = torch.from_numpy(rng.normal(0, 1, (int(empty.sum()), v.shape[2])).astype(np.float32)).to(DEV)
    return st


def slot_parts(fine, k):
    """the k * k part states of the coarse size: part j holds slot j = Morton(dx, dy) of every coarse pixel, cleared outside the film"""
    H, W = fine["n"].shape
    Hc, Wc = coarse(H, k), coarse(W, k)
    parts = []
    for j in range(k * k):
        dx, dy = morton(j)
        part = {}
        for key, v in fine.items():
            if v is None:
                part[key] = None
                continue
            p = torch.zeros((Hc, Wc) + tuple(v.shape[2:]), dtype=v.dtype, device=DEV)
            sub = v[dy::k, dx::k]
            p[:sub.shape[0], :sub.shape[1]] = sub
            part[key] = p
        parts.append(part)
    return parts


class Guarded:
    """dst images with GUARD sentinel floats behind each, holding NaN (counts: -1) before the call: dst is written, never read"""

    def __init__(self):
        self.bufs = []

    def image(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        buf = torch.full((n + GUARD,), SENTINEL if dtype == torch.float32 else int(SENTINEL), dtype=dtype, device=DEV)
        buf[:n] = float("nan") if dtype == torch.float32 else -1
        self.bufs.append((buf, n))
        return buf[:n].view(shape)

    def state(self, Hc, Wc, ch, mm, film, own=True):
        st = {"n": self.image((Hc, Wc), torch.int32) if own else None}
        for f in ("mean", "m2", "m3")[:mm] + (("film_mean", "film_m2") if film else ()):
            st[f] = self.image((Hc, Wc, ch))
        return st

    def check(self):
        for buf, n in self.bufs:
            tail = buf[n:].cpu().numpy()
            assert (tail == (SENTINEL if tail.dtype == np.float32 else int(SENTINEL))).all(), "a guard band behind a dst plane was written"


def pool_one(api, fine, k, ch, mm, transform, prepass=False, guard=None):
    """one own-count entry; returns (dst state, (mean_corr, discriminator) or None)"""
    H, W = fine["n"].shape
    Hc, Wc = coarse(H, k), coarse(W, k)
    g = guard if guard is not None else Guarded()
    dst = g.state(Hc, Wc, ch, mm, transform)
    pre = (g.image((Hc, Wc, ch)), g.image((Hc, Wc, ch))) if prepass else None
    api.pool_statistics(W, H, k, [api.make_pool_entry(dst, fine, ch, mm, prepass_into=pre)])
    torch.cuda.synchronize()
    if guard is None:
        g.check()
    return dst, pre


def prepass_of(api, st, ch):
    mc, dc = torch.zeros_like(st["mean"]), torch.zeros_like(st["mean"])
    args, keep = api.make_filter_args(n=[st["n"]], mean=[st["mean"]], m2=[st["m2"]], m3=[st["m3"]], film=[st["mean"]],
                                      mean_corr=[mc], disc=[dc], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
    api.prepass(args, ch)
    torch.cuda.synchronize()
    return mc, dc


# ---------------------------------------------------------------- 1. the definition, bit for bit
FILMS = [(8, 8, "edge"), (8, 8, "scene"), (7, 3, "edge"), (7, 3, "scene"), (18, 10, "scene")]


@pytest.mark.parametrize("W,H,kind", FILMS)
@pytest.mark.parametrize("ch,mm,transform", SIX)
@pytest.mark.parametrize("k", KS)
def test_pool_is_the_morton_tree_of_two_part_combines(gpu, k, ch, mm, transform, W, H, kind):
    api = gpu
    smp, avail = film_stream(kind, ch, W, H)
    rng = np.random.default_rng(1000 * k + W)
    cnt, cases = planted_counts(rng, avail, k)
    fine = add_payload(rng, accumulate_ragged(api, smp, np.zeros_like(cnt), cnt, transform, mm), cnt)
    before = to_np(fine)
    keys = ["n"] + fields_of(mm, transform)
    got, pre = pool_one(api, {key: fine[key] for key in keys}, k, ch, mm, transform, prepass=mm == 3)
    Hc, Wc = coarse(H, k), coarse(W, k)
    assert tuple(got["n"].shape) == (Hc, Wc) and ((W, H, k) != (18, 10, 8) or (Wc, Hc) == (3, 2))
    mc2, dc2 = torch.zeros(Hc, Wc, ch, device=DEV), torch.zeros(Hc, Wc, ch, device=DEV)
    ref = tree(api, Wc, Hc, slot_parts(fine, k), ch, mm, (mc2, dc2) if mm == 3 else None)
    torch.cuda.synchronize()
    same_bits({key: got[key] for key in keys}, ref, "k = %d" % k)        # every pixel, every plane, n
    if mm == 3:
        assert np.array_equal(bits(pre[0]), bits(mc2)) and np.array_equal(bits(pre[1]), bits(dc2))
    same_bits(before, to_np(fine), "src")                                  # the fine film is read only


# ---------------------------------------------------------------- 2. exact cases
@pytest.mark.parametrize("W,H", [(7, 3), (18, 10), (16, 16)])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("k", KS)
def test_exact_cases_bit_for_bit(gpu, k, ch, W, H):
    api = gpu
    rng = np.random.default_rng(17 * k + W + ch)
    cnt, cases = planted_counts(rng, np.full((H, W), 40, np.int32), k)
    fine = random_state(rng, H, W, ch, True, cnt)
    before = to_np(fine)
    guard = Guarded()
    got, _ = pool_one(api, fine, k, ch, 3, True, guard=guard)
    guard.check()
    same_bits(before, to_np(fine), "src")
    got = to_np(got)
    Hc, Wc = coarse(H, k), coarse(W, k)
    pad = np.zeros((Hc * k, Wc * k), np.int64)
    pad[:H, :W] = cnt
    blocks = pad.reshape(Hc, k, Wc, k)
    assert np.array_equal(got["n"], blocks.sum(axis=(1, 3)))
    live = (blocks > 0).sum(axis=(1, 3))
    seen = {"empty": 0, "one": 0, "one_not_slot0": 0}
    for Y in range(Hc):
        for X in range(Wc):
            if live[Y, X] > 1:
                continue
            if live[Y, X] == 0:
                x, y = X * k, Y * k                                  # slot 0: the payload planted there survives
                seen["empty"] += 1
            else:
                dy, dx = np.argwhere(blocks[Y, :, X, :] > 0)[0]
                x, y = X * k + dx, Y * k + dy
                seen["one"] += 1
                seen["one_not_slot0"] += (dx, dy) != (0, 0)
            for f in ("mean", "m2", "m3", "film_mean", "film_m2"):
                assert np.array_equal(bits(got[f][Y, X]), bits(before[f][y, x])), (f, X, Y)
            assert np.abs(before["mean"][y, x]).sum() > 0
    if Wc * Hc >= 4:
        assert seen["empty"] >= len(cases["empty"]) > 0 and seen["one_not_slot0"] >= len(cases["one_live_not_slot0"]) > 0, seen
    for (X, Y) in cases["slot0_empty"]:
        assert cnt[Y * k, X * k] == 0 and got["n"][Y, X] > 0


# ---------------------------------------------------------------- 3. composition on the device
@pytest.mark.parametrize("W,H", [(7, 3), (18, 10)])
def test_pooling_composes_bit_for_bit(gpu, W, H):
    """pool_2 twice == pool_4, pool_2 of pool_4 == pool_4 of pool_2 == pool_8: partial blocks included, epilogue included"""
    api = gpu
    ch, mm, transform = 3, 3, True
    smp, avail = film_stream("scene", ch, W, H)
    rng = np.random.default_rng(W)
    cnt, _ = planted_counts(rng, avail, 2)
    fine = add_payload(rng, accumulate_ragged(api, smp, np.zeros_like(cnt), cnt, transform, mm), cnt)
    p = {k: pool_one(api, fine, k, ch, mm, transform, prepass=True) for k in KS}
    for a, b in ((2, 2), (2, 4), (4, 2)):
        again, pre = pool_one(api, p[b][0], a, ch, mm, transform, prepass=True)
        same_bits(again, p[a * b][0], "pool_%d(pool_%d)" % (a, b))
        assert np.array_equal(bits(pre[0]), bits(p[a * b][1][0])) and np.array_equal(bits(pre[1]), bits(p[a * b][1][1]))
    assert np.array_equal(to_np(p[8][0])["n"].sum(), cnt.sum())


# ---------------------------------------------------------------- 4. borrowed counts
@pytest.mark.parametrize("W,H", [(7, 3), (18, 10)])
@pytest.mark.parametrize("k", KS)
def test_borrowed_counts_are_the_owners_counts(gpu, k, W, H):
    """a "film" image and a 1-channel mean pooled with count_of = the bits of the same planes pooled as own-count entries whose n is a
    copy of the owner's; the owner may stand anywhere in the call"""
    api = gpu
    rng = np.random.default_rng(31 + k)
    cnt, _ = planted_counts(rng, np.full((H, W), 30, np.int32), k)
    rad = random_state(rng, H, W, 3, True, cnt)
    film = {"mean": torch.from_numpy(rng.normal(0, 1, (H, W, 3)).astype(np.float32)).to(DEV)}
    depth = {"mean": torch.from_numpy(rng.normal(0, 1, (H, W, 1)).astype(np.float32)).to(DEV)}
    Hc, Wc = coarse(H, k), coarse(W, k)
    outs = []
    for owner_at in (0, 2):
        g = Guarded()
        d_rad, d_film, d_depth = g.state(Hc, Wc, 3, 3, True), g.state(Hc, Wc, 3, 1, False, own=False), g.state(Hc, Wc, 1, 1, False, own=False)
        es = [api.make_pool_entry(d_film, film, 3, 1, count_of=owner_at), api.make_pool_entry(d_depth, depth, 1, 1, count_of=owner_at)]
        es.insert(owner_at, api.make_pool_entry(d_rad, rad, 3, 3))
        api.pool_statistics(W, H, k, es)
        torch.cuda.synchronize()
        g.check()
        outs.append((d_rad, d_film, d_depth))
    same_bits(outs[0][0], outs[1][0], "owner first / last"), same_bits(outs[0][1], outs[1][1], "film"), same_bits(outs[0][2], outs[1][2], "depth")
    own_film, _ = pool_one(api, {"n": rad["n"].clone(), "mean": film["mean"]}, k, 3, 1, False)
    own_depth, _ = pool_one(api, {"n": rad["n"].clone(), "mean": depth["mean"]}, k, 1, 1, False)
    assert np.array_equal(bits(outs[0][1]["mean"]), bits(own_film["mean"]))
    assert np.array_equal(bits(outs[0][2]["mean"]), bits(own_depth["mean"]))
    assert np.array_equal(bits(own_film["n"]), bits(outs[0][0]["n"]))
    alone, _ = pool_one(api, rad, k, 3, 3, True)
    same_bits(alone, outs[0][0], "the owner, alone")


# ---------------------------------------------------------------- 5. the epilogue
@pytest.mark.parametrize("spec", [{}, {"dof": 1}, {"small_n": 1}, {"sides": 1}], ids=["default", "welch", "small_n_exclude", "one_sided"])
@pytest.mark.parametrize("ch", [1, 3])
def test_epilogue_is_the_prepass_of_the_pooled_images(gpu, ch, spec):
    api = gpu
    W, H, k = 18, 10, 4
    smp, avail = film_stream("scene", ch, W, H)
    rng = np.random.default_rng(ch)
    cnt, _ = planted_counts(rng, np.minimum(avail, 3), k)          # n = 0, 1, 2 ... per coarse pixel: every branch of the pre-pass
    fine = accumulate_ragged(api, smp, np.zeros_like(cnt), cnt, False, 3)
    try:
        if spec:
            api.set_filter_spec(**spec)
        got, pre = pool_one(api, fine, k, ch, 3, False, prepass=True)
        mc, dc = prepass_of(api, got, ch)
    finally:
        api.set_filter_spec()
    n = to_np(got)["n"]
    assert (n == 0).any() and (n >= 2).any()
    assert np.array_equal(bits(pre[0]), bits(mc)) and np.array_equal(bits(pre[1]), bits(dc))


# ---------------------------------------------------------------- 6. several entries in one call
def film_set(api, rng, W, H, k, fused=False):
    from statmc_amd import film
    types = ("radiance", "normal", "albedo", "depth", "materialid")
    fs = film.FilmStats(W, H, DEV, types=types, g_buffers=("normal", "albedo"), fused_prepass=fused)
    cnt, _ = planted_counts(rng, np.full((H, W), 25, np.int32), k)
    for t in types:
        cfg = film.STAT_TYPES[t]
        st = random_state(rng, H, W, cfg["channels"], cfg["transform"], cnt)
        st["m2"].abs_()
        for key, v in fs.state[t].items():
            if v is not None:
                v.copy_(st[key])
    fs.film.copy_(torch.from_numpy(rng.random((H, W, 3)).astype(np.float32)))
    return fs, cnt


@pytest.mark.parametrize("W,H", [(7, 3), (18, 10), (64, 48)])
@pytest.mark.parametrize("k", KS)
def test_one_call_with_the_whole_film_set_equals_one_call_per_entry(gpu, k, W, H):
    """the 11-channel set plus "film" -- six entries, three instantiations -- in one launch; 64 x 48 takes the dwordx2 loads"""
    from statmc_amd import film
    api = gpu
    fs, cnt = film_set(api, np.random.default_rng(W + k), W, H, k)
    pooled = fs.pooled(k)
    torch.cuda.synchronize()
    for t in fs.types:
        cfg = film.STAT_TYPES[t]
        keys = ["n"] + fields_of(cfg["max_moment"], cfg["transform"])
        alone, _ = pool_one(api, {key: fs.state[t][key] for key in keys}, k, cfg["channels"], cfg["max_moment"], cfg["transform"])
        same_bits(alone, pooled.state[t], t)
    alone, _ = pool_one(api, {"n": fs.state["radiance"]["n"], "mean": fs.film}, k, 3, 1, False)
    assert np.array_equal(bits(alone["mean"]), bits(pooled.film))


def test_unaligned_planes_take_the_scalar_loads_and_leave_the_same_bits(gpu):
    api = gpu
    W, H, k = 64, 48, 4
    rng = np.random.default_rng(5)
    cnt, _ = planted_counts(rng, np.full((H, W), 25, np.int32), k)
    fine = random_state(rng, H, W, 3, True, cnt)
    aligned, _ = pool_one(api, fine, k, 3, 3, True)
    shifted = {}
    for key, v in fine.items():
        buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=DEV)
        shifted[key] = buf[1:].view(v.shape)
        shifted[key].copy_(v)
        assert shifted[key].data_ptr() % 8 == 4
    unaligned, _ = pool_one(api, shifted, k, 3, 3, True)
    same_bits(aligned, unaligned, "dwordx2 / scalar loads")


# ---------------------------------------------------------------- 7. the union of the samples
@pytest.mark.parametrize("ch,mm,transform", SIX)
@pytest.mark.parametrize("k", KS)
def test_the_pooled_state_matches_the_union_of_the_blocks_samples(gpu, k, ch, mm, transform):
    """the project's rule: per field at most twice as far (relative L2) from the float64 two-pass moments of all samples of the block
    as the sequential accumulation of those samples in slot order, + 1e-6"""
    api = gpu
    W, H = 18, 10
    smp, avail = film_stream("scene", ch, W, H)
    S = smp.shape[0]
    cnt, _ = planted_counts(np.random.default_rng(k), avail, k)
    fine = accumulate_ragged(api, smp, np.zeros_like(cnt), cnt, transform, mm)
    got, _ = pool_one(api, {key: fine[key] for key in ["n"] + fields_of(mm, transform)}, k, ch, mm, transform)
    Hc, Wc = coarse(H, k), coarse(W, k)
    # every block's samples as one pixel's stream, in slot order
    block = np.zeros((S * k * k, Hc, Wc, ch), np.float32)
    total = np.zeros((Hc, Wc), np.int32)
    for Y in range(Hc):
        for X in range(Wc):
            run = []
            for j in range(k * k):
                dx, dy = morton(j)
                x, y = X * k + dx, Y * k + dy
                if x < W and y < H:
                    run.append(smp[:cnt[y, x], y, x])
            run = np.concatenate(run) if run else np.zeros((0, ch), np.float32)
            block[:len(run), Y, X] = run
            total[Y, X] = len(run)
    seq = accumulate_ragged(api, block, np.zeros_like(total), total, transform, mm)
    got, sq = to_np(got), to_np(seq)
    assert np.array_equal(got["n"], total) and np.array_equal(sq["n"], total)
    check_union_rule(got, sq, union64(block, total, transform), fields_of(mm, transform), "pool k = %d" % k)


# ---------------------------------------------------------------- 8. a stream row
def pool_case(api, name, k=4):
    """7 x 3: an own-count entry with film images of its own and the epilogue, and a "film" entry that borrows its counts"""
    W, H = 7, 3
    Hc, Wc = coarse(H, k), coarse(W, k)
    case = Case(name, seed=k)
    rng = np.random.default_rng(61)
    n = rng.integers(0, 40, (H, W)).astype(np.int32)
    n[0, :3] = 0
    src = {"n": case.live(n)}
    for f in ("mean", "m2", "m3", "film_mean", "film_m2"):
        src[f] = case.live(np.abs(rng.normal(0, 1, (H, W, 3))).astype(np.float32))
    film = {"mean": case.live(rng.random((H, W, 3)).astype(np.float32))}
    dst = {"n": case.state_image((Hc, Wc), np.int32, out="n")}
    for f in ("mean", "m2", "m3", "film_mean", "film_m2"):
        dst[f] = case.state_image((Hc, Wc, 3), np.float32, out=f)
    pre = (case.state_image((Hc, Wc, 3), np.float32, out="mean_corr"), case.state_image((Hc, Wc, 3), np.float32, out="discriminator"))
    dfilm = {"mean": case.state_image((Hc, Wc, 3), np.float32, out="film")}
    entries = [api.make_pool_entry(dst, src, 3, 3, prepass_into=pre), api.make_pool_entry(dfilm, film, 3, 1, count_of=0)]
    case.call = lambda stream: api.pool_statistics(W, H, k, entries, stream=stream)
    return case


def test_pool_runs_on_its_stream(gpu, side):
    """the entry enqueued on a side stream behind a closed gate, its inputs copied in behind the gate: the null-stream run's bits"""
    api = gpu
    s, gate = side
    case = pool_case(api, "pool_statistics")
    want = run_on_null_stream(case)
    got = run_gated(api, case, s, gate)
    assert_same_bits(case, got, want, "gated on the side stream against the null-stream run")
    assert (case.res("n") >= 0).all() and np.isfinite(case.res("mean")).all()


# ---------------------------------------------------------------- 9. host layers
@pytest.mark.parametrize("k", KS)
def test_filmstats_pooled_and_its_denoise(gpu, k):
    """FilmStats.pooled(k) leaves the bits of the direct call, with fused_prepass the epilogue's mean-corr / discriminator, and its
    denoise() is api.filter_f32x3 on the pooled images"""
    from statmc_amd import film
    api = gpu
    W, H = 61, 37
    fs, cnt = film_set(api, np.random.default_rng(3 * k), W, H, k, fused=True)
    for t in fs.types:                     # G-buffers that the window filter can weigh
        if t != "radiance":
            fs.state[t]["mean"].copy_(torch.rand_like(fs.state[t]["mean"]))
    pooled = fs.pooled(k)
    Wc, Hc = api.pooled_size(W, H, k)
    assert (pooled.width, pooled.height) == (Wc, Hc) and pooled._prepass_current is not None
    rad, pre = pool_one(api, fs.state["radiance"], k, 3, 3, True, prepass=True)
    same_bits(rad, pooled.state["radiance"], "radiance")
    assert np.array_equal(bits(pre[0]), bits(pooled.mean_corr)) and np.array_equal(bits(pre[1]), bits(pooled.disc))
    out = pooled.denoise().clone()
    direct = {}
    for t in ("normal", "albedo"):
        direct[t], _ = pool_one(api, {"n": fs.state[t]["n"], "mean": fs.state[t]["mean"]}, k, 3, 1, False)
    mc, dc, ff = (torch.zeros(Hc, Wc, 3, device=DEV) for _ in range(3))
    args, keep = api.make_filter_args(n=[rad["n"]], mean=[rad["mean"]], m2=[rad["m2"]], m3=[rad["m3"]], film=[rad["film_mean"]],
                                      mean_corr=[mc], disc=[dc], film_filtered=[ff], g_buffers=[direct["normal"]["mean"], direct["albedo"]["mean"]],
                                      g_sds=[SD_NORMAL, SD_ALBEDO], filter_sd=FILTER_SD, radius=RADIUS)
    api.filter_f32x3(args)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), bits(ff)) and np.isfinite(out.cpu().numpy()).any()
    assert np.array_equal(bits(mc), bits(pooled.mean_corr))


def test_estimator_pool_statistics(gpu):
    """tests/cpp/test_pool_statistics.cpp: Estimator::PoolStatistics + coarse.Denoise() against the C entry by hand"""
    from statmc_amd import build
    build.build_tools()
    for W, H, k in ((37, 23, 4), (30, 18, 2), (21, 40, 8)):
        r = subprocess.run([build.POOL_BIN, str(W), str(H), str(k)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "pool statistics OK" in r.stdout, r.stdout + r.stderr


def test_offline_tool_pools_a_dump(gpu, tmp_path):
    """statmc_denoise --pool 2 on a small for-ours dump: the coarse-size PFMs it writes are the Python path's bits -- the pooled
    statistics, the G-buffer means pooled with t0-b0-n, the pooled "film", and the film-f of the coarse film"""
    from statmc_amd import build, pfm
    api = gpu
    exe = build.build_tools()
    W, H, S, k = 45, 26, 8, 2
    Wc, Hc = api.pooled_size(W, H, k)
    rng = np.random.default_rng(9)
    cnt = rng.integers(0, S + 1, (H, W)).astype(np.int32)
    cnt[:2, :2] = 0
    rad = random_state(rng, H, W, 3, False, cnt)
    rad["m2"].abs_()
    img = lambda: torch.from_numpy(rng.random((H, W, 3)).astype(np.float32)).to(DEV)
    film, normal, albedo = img(), img(), img()
    stem, out = str(tmp_path / "fine"), str(tmp_path / "coarse")
    dump = {"film": film, "t0-b0-n": rad["n"], "t0-b0-mean": rad["mean"], "t0-b0-m2": rad["m2"], "t0-b0-m3": rad["m3"],
            "t1-b0-film-mean": normal, "t2-b0-film-mean": albedo}
    for name, t in dump.items():
        pfm.write_pfm("%s-%d-%s.pfm" % (stem, S, name), t.cpu().numpy())
    names = ["film-f", "t0-b0-n", "t0-b0-mean", "t0-b0-m2", "t0-b0-m3", "t1-b0-film-mean", "t2-b0-film-mean", "film", "t0-b0-mean-corr"]
    r = subprocess.run([exe, "--stem", stem, "--spp", str(S), "--pool", str(k), "--output-stem", out, "--filtersd", str(FILTER_SD),
                        "--filterradius", str(RADIUS), "--output", ",".join(names)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "pool: %d x %d pooled %d x %d into %d x %d" % (W, H, k, k, Wc, Hc) in r.stdout
    rd = lambda name: pfm.read_pfm("%s-%d-%s.pfm" % (out, S, name))
    # the Python path
    g = Guarded()
    d_rad = g.state(Hc, Wc, 3, 3, False)
    d_film, d_normal, d_albedo = (g.state(Hc, Wc, 3, 1, False, own=False) for _ in range(3))
    api.pool_statistics(W, H, k, [api.make_pool_entry(d_rad, {key: rad[key] for key in ("n", "mean", "m2", "m3")}, 3, 3),
                                  api.make_pool_entry(d_normal, {"mean": normal}, 3, 1, count_of=0),
                                  api.make_pool_entry(d_albedo, {"mean": albedo}, 3, 1, count_of=0),
                                  api.make_pool_entry(d_film, {"mean": film}, 3, 1, count_of=0)])
    mc, dc, ff = (torch.zeros(Hc, Wc, 3, device=DEV) for _ in range(3))
    args, keep = api.make_filter_args(n=[d_rad["n"]], mean=[d_rad["mean"]], m2=[d_rad["m2"]], m3=[d_rad["m3"]], film=[d_film["mean"]],
                                      mean_corr=[mc], disc=[dc], film_filtered=[ff], g_buffers=[d_normal["mean"], d_albedo["mean"]],
                                      g_sds=[SD_NORMAL, SD_ALBEDO], filter_sd=FILTER_SD, radius=RADIUS)
    api.filter_f32x3(args)
    torch.cuda.synchronize()
    g.check()
    want = {"film-f": ff, "t0-b0-mean": d_rad["mean"], "t0-b0-m2": d_rad["m2"], "t0-b0-m3": d_rad["m3"], "t1-b0-film-mean": d_normal["mean"],
            "t2-b0-film-mean": d_albedo["mean"], "film": d_film["mean"], "t0-b0-mean-corr": mc}
    for name, t in want.items():
        got = rd(name)
        assert got.shape[:2] == (Hc, Wc), name
        assert np.array_equal(bits(got.astype(np.float32)), bits(t)), name
    assert np.array_equal(rd("t0-b0-n").reshape(Hc, Wc), d_rad["n"].cpu().numpy().astype(np.float32))
    # argument errors
    r = subprocess.run([exe, "--stem", stem, "--spp", str(S), "--pool", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--pool" in r.stderr
    r = subprocess.run([exe, "--stem", stem, "--spp", str(S), "--pool", "2", "--grid", "1x1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--grid" in r.stderr
