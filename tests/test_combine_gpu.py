"""statmc_combine_statistics on the GPU (include/statmc.h): two independently accumulated parts of every pixel's samples,
combined, against the union of the samples, against the float64 restatement of the formulas (tests/test_combine_cpu.py),
its exact cases, borrowed counts, aliasing, the pre-pass epilogue, validation, FilmStats.combine_ end to end at 1080p and
the offline tool's --combine."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import FILTER_SD, RADIUS, SD_ALBEDO, SD_NORMAL, edge_case_stream, rel_l2
from test_combine_cpu import combine64, two_pass64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G_DR = [-0.5 / SD_NORMAL ** 2, -0.5 / SD_ALBEDO ** 2]
FIELDS = ("mean", "m2", "m3", "film_mean", "film_m2")


def fields_of(max_moment, transform):
    f = ["mean", "m2", "m3"][:max_moment]
    return f + (["film_mean", "film_m2"] if transform else [])


def new_state(h, w, c, transform):
    from statmc_amd import film
    return film.new_state(h, w, c, DEV, transform=transform)


def accumulate_ragged(api, samples, first, count, transform, max_moment):
    """State of samples[first[p] : first[p] + count[p], p] for every pixel p, accumulated by statmc_accumulate: the pixels
    of one count go through one call as a one-row image (the update is per pixel)."""
    S, H, W, Ch = samples.shape
    st = new_state(H, W, Ch, transform)
    flat_first, flat_count = first.reshape(-1), count.reshape(-1)
    smp = samples.reshape(S, H * W, Ch)
    for c in sorted(set(int(v) for v in flat_count if v > 0)):
        pix = np.nonzero(flat_count == c)[0]
        idx = flat_first[pix][None, :] + np.arange(c)[:, None]             # [c, P]
        part = np.ascontiguousarray(smp[idx, pix[None, :]])[:, None]       # [c, 1, P, Ch]
        sub = new_state(1, len(pix), Ch, transform)
        api.accumulate(len(pix), 1, [api.make_stat_type(torch.from_numpy(part).to(DEV), sub, transform, max_moment)])
        ys, xs = torch.from_numpy(pix // W).to(DEV), torch.from_numpy(pix % W).to(DEV)
        for k, v in sub.items():
            if v is not None:
                st[k][ys, xs] = v[0]
    torch.cuda.synchronize()
    return st


def to_np(st):
    return {k: v.cpu().numpy() for k, v in st.items() if v is not None}


def clone(st):
    return {k: (v.clone() if v is not None else None) for k, v in st.items()}


def union64(samples, count, transform):
    """float64 two-pass moments of every pixel's samples[:count[p]]: mean / m2 / m3 of the (Box-Cox) values, film_mean /
    film_m2 of the raw ones."""
    S, H, W, Ch = samples.shape
    out = {k: np.zeros((H, W, Ch)) for k in FIELDS}
    for y in range(H):
        for x in range(W):
            n = count[y, x]
            if n == 0:
                continue
            raw = samples[:n, y, x].astype(np.float64)
            v = ((np.sqrt(samples[:n, y, x]) - np.float32(1)) / np.float32(.5)).astype(np.float64) if transform else raw
            out["mean"][y, x], out["m2"][y, x], out["m3"][y, x] = two_pass64(v)
            fm, f2, _ = two_pass64(raw)
            out["film_mean"][y, x], out["film_m2"][y, x] = fm, f2
    return out


def entry(api, dst, src, ch, mm, **kw):
    return api.make_combine_entry(dst, src, ch, mm, **kw)


def case_streams(kind, ch):
    """(samples [S, H, W, ch], count [H, W], split [H, W]): the edge cases of SURVEY 8c or a synthetic scene; every pixel's
    samples split at an uneven point, 0 and all of them included."""
    rng = np.random.default_rng(5)
    if kind == "edge":
        count, smp = edge_case_stream()
    else:
        from statmc_amd import synthetic
        smp = synthetic.Scene(20, 6, seed=3).samples(18, seed=4, features=("radiance",))["radiance"].numpy()
        count = np.full(smp.shape[1:3], smp.shape[0], np.int32)
    smp = np.ascontiguousarray(smp[..., :ch])
    split = rng.integers(0, count + 1).astype(np.int32)
    split.reshape(-1)[0::7] = 0
    split.reshape(-1)[3::7] = count.reshape(-1)[3::7]
    return smp, count, split


@pytest.mark.parametrize("kind", ["edge", "scene"])
@pytest.mark.parametrize("ch,mm,transform", [(3, 3, True), (3, 3, False), (3, 2, True), (3, 1, False), (1, 3, True),
                                             (1, 2, False), (1, 1, True), (1, 1, False), (3, 2, False), (3, 1, True)])
def test_combine_matches_the_union_and_the_formula(gpu, kind, ch, mm, transform):
    api = gpu
    smp, count, split = case_streams(kind, ch)
    zero = np.zeros_like(count)
    A = accumulate_ragged(api, smp, zero, split, transform, mm)
    B = accumulate_ragged(api, smp, split, count - split, transform, mm)
    seq = accumulate_ragged(api, smp, zero, count, transform, mm)
    A0, B0 = to_np(A), to_np(B)
    H, W = count.shape
    api.combine_statistics(W, H, [entry(api, A, B, ch, mm)])
    torch.cuda.synchronize()
    got, sq = to_np(A), to_np(seq)
    assert np.array_equal(got["n"], sq["n"]) and np.array_equal(got["n"], count)
    ref = union64(smp, count, transform)
    fields = fields_of(mm, transform)
    # 1. against the union of the samples
    for k in fields:
        e_seq = rel_l2(sq[k], ref[k])
        assert rel_l2(got[k], ref[k]) <= 2 * e_seq + 1e-6, (k, rel_l2(got[k], ref[k]), e_seq)
    if kind == "edge":    # zeros (Box-Cox -2), constants, n = 1, and the pixels one part has no sample of: exact
        rows = [3, 4, 6]
        for k in fields:
            assert np.array_equal(got[k][rows], sq[k][rows]), k
        empty = (split == 0) | (split == count)
        for k in fields:
            assert np.array_equal(got[k][empty], sq[k][empty]), k
    # 2. against the float64 restatement on the same fp32 inputs
    n64, want = combine64(A0["n"], {k: A0[k].astype(np.float64) for k in ("mean", "m2", "m3") if k in fields},
                          B0["n"], {k: B0[k].astype(np.float64) for k in ("mean", "m2", "m3") if k in fields}, mm)
    assert np.array_equal(n64, got["n"])
    for k in [f for f in fields if not f.startswith("film")]:
        assert rel_l2(got[k], want[k]) <= 1e-6, k
    if transform:
        _, wf = combine64(A0["n"], {"mean": A0["film_mean"].astype(np.float64), "m2": A0["film_m2"].astype(np.float64)},
                          B0["n"], {"mean": B0["film_mean"].astype(np.float64), "m2": B0["film_m2"].astype(np.float64)}, 2)
        assert rel_l2(got["film_mean"], wf["mean"]) <= 1e-6
        assert rel_l2(got["film_m2"], wf["m2"]) <= 1e-6


def random_state(rng, H, W, ch, transform, n):
    st = new_state(H, W, ch, transform)
    st["n"].copy_(torch.from_numpy(n))
    for k, v in st.items():
        if k != "n" and v is not None:
            v.copy_(torch.from_numpy(rng.normal(0, 1, v.shape).astype(np.float32)))
    return st


@pytest.mark.parametrize("W,H", [(8, 8), (7, 3)])   # 4-pixel groups as dwordx4, and a scalar tail
@pytest.mark.parametrize("ch", [1, 3])
def test_exact_cases_bit_for_bit(gpu, W, H, ch):
    """nB = 0 leaves dst's bits, nA = 0 copies src's bits -- per pixel, both in one image beside ordinary pixels."""
    api = gpu
    rng = np.random.default_rng(11)
    nA = rng.integers(1, 50, (H, W)).astype(np.int32)
    nB = rng.integers(1, 50, (H, W)).astype(np.int32)
    case = rng.integers(0, 3, (H, W))
    nA[case == 1] = 0
    nB[case == 2] = 0
    nB[0, 0] = 0
    nA[0, 1] = 0
    A, B = random_state(rng, H, W, ch, True, nA), random_state(rng, H, W, ch, True, nB)
    A0, B0 = to_np(A), to_np(B)
    api.combine_statistics(W, H, [entry(api, A, B, ch, 3)])
    torch.cuda.synchronize()
    got = to_np(A)
    assert np.array_equal(got["n"], nA + nB)
    keep, take = nB == 0, (nB > 0) & (nA == 0)
    for k in FIELDS:
        assert np.array_equal(got[k][keep].view(np.int32), A0[k][keep].view(np.int32)), k
        assert np.array_equal(got[k][take].view(np.int32), B0[k][take].view(np.int32)), k
        mixed = ~(keep | take)
        assert not np.array_equal(got[k][mixed], A0[k][mixed]), k
    assert np.array_equal(to_np(B)["n"], nB)     # src is read only
    for k in FIELDS:
        assert np.array_equal(to_np(B)[k], B0[k])


def test_borrowed_counts_are_the_counts_before_the_call(gpu):
    """film and G-buffer means weighed with the radiance counts: the same bits whether the borrowing entries come before or
    after their count owner, and the formula's values with the owner's counts from before the call."""
    api = gpu
    rng = np.random.default_rng(2)
    H, W = 9, 13
    nA = rng.integers(0, 40, (H, W)).astype(np.int32)
    nB = rng.integers(0, 40, (H, W)).astype(np.int32)
    radA, radB = random_state(rng, H, W, 3, True, nA), random_state(rng, H, W, 3, True, nB)
    mk = lambda: {"mean": torch.from_numpy(rng.normal(0, 1, (H, W, 3)).astype(np.float32)).to(DEV)}
    filmA, filmB, nrmA, nrmB = mk(), mk(), mk(), mk()
    dep = lambda: {"mean": torch.from_numpy(rng.normal(0, 1, (H, W, 1)).astype(np.float32)).to(DEV)}
    depA, depB = dep(), dep()
    outs = []
    for order in ("after", "before"):
        ra, fa, na, da = clone(radA), clone(filmA), clone(nrmA), clone(depA)
        if order == "after":
            es = [entry(api, ra, radB, 3, 3), entry(api, fa, filmB, 3, 1, count_of=0), entry(api, na, nrmB, 3, 1, count_of=0),
                  entry(api, da, depB, 1, 1, count_of=0)]
        else:
            es = [entry(api, fa, filmB, 3, 1, count_of=3), entry(api, na, nrmB, 3, 1, count_of=3),
                  entry(api, da, depB, 1, 1, count_of=3), entry(api, ra, radB, 3, 3)]
        api.combine_statistics(W, H, es)
        torch.cuda.synchronize()
        outs.append((to_np(ra), fa["mean"].cpu().numpy(), na["mean"].cpu().numpy(), da["mean"].cpu().numpy()))
    (r0, f0, n0, d0), (r1, f1, n1, d1) = outs
    for k in ("n",) + FIELDS:
        assert np.array_equal(r0[k], r1[k]), k
    assert np.array_equal(f0, f1) and np.array_equal(n0, n1) and np.array_equal(d0, d1)
    assert np.array_equal(r0["n"], nA + nB)
    for got, a, b in ((f0, filmA, filmB), (n0, nrmA, nrmB), (d0, depA, depB)):
        _, want = combine64(nA, {"mean": a["mean"].cpu().numpy().astype(np.float64)}, nB,
                            {"mean": b["mean"].cpu().numpy().astype(np.float64)}, 1)
        assert rel_l2(got, want["mean"]) <= 1e-6


def test_aliased_film_images_are_combined_once(gpu):
    """A non-transform type whose film_mean / film_m2 are its mean / m2 (estimator.cpp:127-137): combined once -- the bits
    of the same entry without film images."""
    api = gpu
    rng = np.random.default_rng(4)
    H, W = 6, 10
    nA = rng.integers(1, 30, (H, W)).astype(np.int32)
    nB = rng.integers(1, 30, (H, W)).astype(np.int32)
    A, B = random_state(rng, H, W, 3, False, nA), random_state(rng, H, W, 3, False, nB)
    A["m2"].abs_()
    B["m2"].abs_()
    A2 = clone(A)
    for s in (A, B):
        s["film_mean"], s["film_m2"] = s["mean"], s["m2"]
    api.combine_statistics(W, H, [entry(api, A, B, 3, 2)])
    api.combine_statistics(W, H, [entry(api, A2, {k: v for k, v in B.items() if not k.startswith("film")}, 3, 2)])
    torch.cuda.synchronize()
    for k in ("n", "mean", "m2"):
        assert torch.equal(A[k], A2[k]), k


@pytest.mark.parametrize("dof", ["pixel", "welch"])
def test_prepass_epilogue_is_the_prepass_of_the_combined_moments(gpu, dof):
    api = gpu
    smp, count, split = case_streams("edge", 3)
    zero = np.zeros_like(count)
    A = accumulate_ragged(api, smp, zero, split, True, 3)
    B = accumulate_ragged(api, smp, split, count - split, True, 3)
    H, W = count.shape
    mc, dc = torch.full((H, W, 3), 7.0, device=DEV), torch.full((H, W, 3), 7.0, device=DEV)
    try:
        if dof == "welch":
            api.set_filter_spec(dof=api.DOF_WELCH)
        api.combine_statistics(W, H, [entry(api, A, B, 3, 3, prepass_into=(mc, dc))])
        mc2, dc2 = torch.zeros_like(mc), torch.zeros_like(dc)
        args, keep = api.make_filter_args(n=[A["n"]], mean=[A["mean"]], m2=[A["m2"]], m3=[A["m3"]], film=[A["film_mean"]],
                                          mean_corr=[mc2], disc=[dc2], film_filtered=[torch.zeros_like(mc)], g_buffers=[])
        api.prepass(args, 3)
        torch.cuda.synchronize()
    finally:
        api.set_filter_spec()
    assert np.array_equal(mc.cpu().numpy().view(np.int32), mc2.cpu().numpy().view(np.int32))
    assert np.array_equal(dc.cpu().numpy().view(np.int32), dc2.cpu().numpy().view(np.int32))


def test_validation(gpu):
    """Every rule of include/statmc.h returns STATMC_ERR_INVALID (and nothing is launched)."""
    api = gpu
    lib = api.load()
    H, W = 4, 8
    mk = lambda: new_state(H, W, 3, True)
    A, B, F1, F2 = mk(), mk(), mk(), mk()
    mc, dc = torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 3, device=DEV)
    film = lambda s: {"mean": s["mean"]}

    def rc(entries, n=None):
        arr = (api.CombineEntry * max(len(entries), 1))(*entries)
        return lib.statmc_combine_statistics(W, H, arr, len(entries) if n is None else n, None)

    ok = entry(api, A, B, 3, 3)
    assert rc([ok]) == api.STATMC_OK
    assert rc([], 0) == api.STATMC_OK
    assert rc([ok] * 17) == api.ERR_INVALID and b"n_entries" in lib.statmc_last_error()
    assert lib.statmc_combine_statistics(W, H, None, 1, None) == api.ERR_INVALID
    bad = []
    e = entry(api, A, B, 3, 3); e.dst.mean = None; bad.append(("null mean", [e]))
    e = entry(api, A, B, 3, 3); e.src.m3 = None; bad.append(("null m3", [e]))
    e = entry(api, A, B, 3, 3); e.dst.n = None; bad.append(("null n", [e]))
    e = entry(api, A, B, 3, 3); e.src.m2 = e.dst.m2; bad.append(("dst == src", [e]))
    e = entry(api, A, B, 3, 3); e.src.n = e.dst.n; bad.append(("n dst == src", [e]))
    e = entry(api, A, B, 3, 3); e.src.film_mean = e.dst.film_mean; bad.append(("film dst == src", [e]))
    e = entry(api, A, B, 3, 3); e.src.channels = 1; bad.append(("channels", [e]))
    e = entry(api, A, B, 3, 3); e.src.max_moment = 2; bad.append(("max_moment", [e]))
    e = entry(api, A, B, 3, 3); e.dst.max_moment = e.src.max_moment = 4; bad.append(("max_moment 4", [e]))
    e = entry(api, A, B, 3, 3); e.dst.film_mean = None; bad.append(("film_m2 without film_mean", [e]))
    e = entry(api, A, B, 3, 3); e.dst.mean_corr = mc.data_ptr(); bad.append(("mean_corr alone", [e]))
    e = entry(api, A, B, 3, 2, prepass_into=(mc, dc)); bad.append(("epilogue needs m3", [e]))
    bad.append(("epilogue needs own counts", [ok, entry(api, F1, F2, 3, 3, count_of=0, prepass_into=(mc, dc))]))
    for k in (-2, 1, 5):
        bad.append(("count_of %d" % k, [entry(api, film(F1), film(F2), 3, 1, count_of=k), ok]
                    if k != 1 else [ok, entry(api, film(F1), film(F2), 3, 1, count_of=1)]))
    bad.append(("borrow from a borrower", [ok, entry(api, film(F1), film(F2), 3, 1, count_of=0),
                                           entry(api, film(A), film(B), 3, 1, count_of=1)]))
    e = entry(api, film(F1), film(F2), 3, 1, count_of=0); e.dst.n = F1["n"].data_ptr()
    bad.append(("borrower with n", [ok, e]))
    bad.append(("two owners of one count image", [ok, entry(api, A, F2, 3, 3)]))
    for what, es in bad:
        assert rc(es) == api.ERR_INVALID, what
    torch.cuda.synchronize()


def test_filmstats_combine_end_to_end_1080p(gpu, oracle):
    """256 spp split 128 + 128 at 1920 x 1080: FilmStats.combine_ + the filter against the oracle's pre-pass and filter of
    the combined moments on the strips tests/test_gpu_fullsize.py checks (1e-5), and against the filter of the sequential
    256-spp accumulation over the whole frame (a gross-error bound: gate decisions may flip on last-bit differences)."""
    from statmc_amd import film, synthetic
    W, H = 1920, 1080
    scene = synthetic.Scene(W, H, seed=1, device=DEV)
    parts = [film.FilmStats(W, H, DEV), film.FilmStats(W, H, DEV, fused_prepass=True), film.FilmStats(W, H, DEV)]
    seq, fa, fb = parts[0], parts[1], parts[2]
    for k, seed in enumerate((2, 3)):
        smp = scene.samples(128, seed=seed, features=("radiance", "normal", "albedo"))
        seq.accumulate(smp)
        (fa if k == 0 else fb).accumulate(smp)
        del smp
    fa.combine_(fb)
    assert fa._prepass_current is not None
    for t in fa.types:
        assert torch.equal(fa.state[t]["n"], seq.state[t]["n"])
    out = fa.denoise().clone()
    ref_whole = seq.denoise().clone()
    torch.cuda.synchronize()
    rad = {k: v.cpu().numpy() for k, v in fa.state["radiance"].items()}
    mc, dc = oracle.prepass(rad["n"], rad["mean"], rad["m2"], rad["m3"])
    gbs = [fa.g_buffer("normal").cpu().numpy(), fa.g_buffer("albedo").cpu().numpy()]
    got = out.cpu().numpy()
    for roi in ((0, 530, W, 546), (0, 0, 300, 8), (W - 300, H - 8, W, H)):
        x0, y0, x1, y1 = roi
        ref = oracle.filter_image(mc, dc, rad["film_mean"], gbs, G_DR, -0.5 / FILTER_SD ** 2, RADIUS, roi=roi)[y0:y1, x0:x1]
        for c in range(3):
            assert rel_l2(got[y0:y1, x0:x1, c], ref[..., c]) <= 1e-5, (roi, c)
    whole = ref_whole.cpu().numpy()
    errs = [rel_l2(got[..., c], whole[..., c]) for c in range(3)]
    print("combined 128 + 128 vs sequential 256 spp, whole frame rel L2 per channel: %s" % ["%.3e" % e for e in errs])
    assert max(errs) <= 1e-3


def test_offline_tool_combines_for_ours_dumps(gpu, oracle, tmp_path):
    """Two for-ours dumps of oracle-accumulated halves -> statmc_denoise --combine: the combined dump is test 2's reference,
    and denoising the combined dump on its own gives the same film-f bit for bit."""
    from statmc_amd import build, pfm, synthetic
    from statmc_amd.film import STAT_TYPES
    exe = build.build_tools()
    W, H, S = 96, 40, 8
    scene = synthetic.Scene(W, H, seed=5)
    halves = []
    for seed in (6, 7):
        smp = {k: v.numpy() for k, v in scene.samples(S, seed=seed, features=("radiance", "normal", "albedo")).items()}
        st = {}
        for t in ("radiance", "normal", "albedo"):
            st[t] = oracle.new_state(H, W, 3)
            oracle.accumulate(st[t], smp[t], STAT_TYPES[t]["transform"], STAT_TYPES[t]["max_moment"])
        halves.append(st)
    stems = [str(tmp_path / "a"), str(tmp_path / "b")]
    for stem, st in zip(stems, halves):
        r = st["radiance"]
        dump = {"film": r["film_mean"], "t0-b0-n": r["n"], "t0-b0-mean": r["mean"], "t0-b0-m2": r["m2"], "t0-b0-m3": r["m3"],
                "t1-b0-film-mean": st["normal"]["mean"], "t2-b0-film-mean": st["albedo"]["mean"]}
        for name, img in dump.items():
            pfm.write_pfm("%s-%d-%s.pfm" % (stem, S, name), img)
    pfm.write_pfm("%s-%d-t0-b0-mean-corr.pfm" % (stems[1], S), np.zeros((H, W, 3), np.float32))   # not combined: a note
    pfm.write_pfm("%s-%d-t0-b0-mean-corr.pfm" % (stems[0], S), np.zeros((H, W, 3), np.float32))
    out = str(tmp_path / "o")
    args = ["--filtersd", str(FILTER_SD), "--filterradius", str(RADIUS), "--output", "film-f"]
    r = subprocess.run([exe, "--stem", stems[0], "--spp", str(S), "--combine", stems[1], "--output-stem", out, "--write-combined"]
                       + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "not combined" in r.stdout
    T = 2 * S
    rd = lambda name: pfm.read_pfm("%s-%d-%s.pfm" % (out, T, name))
    a, b = halves[0]["radiance"], halves[1]["radiance"]
    n64, want = combine64(a["n"], {k: a[k].astype(np.float64) for k in ("mean", "m2", "m3")},
                          b["n"], {k: b[k].astype(np.float64) for k in ("mean", "m2", "m3")}, 3)
    assert np.array_equal(rd("t0-b0-n"), n64.astype(np.float32))
    for k in ("mean", "m2", "m3"):
        assert rel_l2(rd("t0-b0-" + k), want[k]) <= 1e-6, k
    for name, key in (("film", None), ("t1-b0-film-mean", "normal"), ("t2-b0-film-mean", "albedo")):
        ia = a["film_mean"] if key is None else halves[0][key]["mean"]
        ib = b["film_mean"] if key is None else halves[1][key]["mean"]
        _, w = combine64(a["n"], {"mean": ia.astype(np.float64)}, b["n"], {"mean": ib.astype(np.float64)}, 1)
        assert rel_l2(rd(name), w["mean"]) <= 1e-6, name
    film_f = rd("film-f")
    assert np.isfinite(film_f).all()
    r = subprocess.run([exe, "--stem", out, "--spp", str(T)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(rd("film-f").view(np.int32), film_f.view(np.int32))
    # a stem without one of the files is refused with that file's name
    os.remove("%s-%d-t2-b0-film-mean.pfm" % (stems[1], S))
    r = subprocess.run([exe, "--stem", stems[0], "--spp", str(S), "--combine", stems[1], "--output-stem", out] + args,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "b-%d-t2-b0-film-mean.pfm" % S in r.stderr
