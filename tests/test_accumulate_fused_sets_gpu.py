"""Every instantiation of the accumulation's type-fused walk: accumulate_fused_kernel<K, M, D> and accumulate_fused_half_kernel<K, M,
FMT> for the eight (K, M) a radiance type and one to four feature types can make, in the three sample formats -- 24 kernels whose
LDS slot layout, transfer pairing, counted wait and ring size are compile-time functions of K, M and FMT.  Every launch is held
against three yardsticks:
  A  bits    the same samples from the same state through the per-type kernel (fp32: the switch at -1; half: the widened samples
             through statmc_accumulate), every plane of every type as int32, and each side asked which kernel it ran;
  B  oracle  oracle.accumulate per type from the same HOST-made starting state: counts, raw-sample moments and every mean-only
             type bit for bit, the Box-Cox moments within TOL, the non-finite elements at the oracle's positions -- and, element
             by element, the bits of the oracle's untransformed chain on the device's own Box-Cox values
             (tests/test_accumulate_boxcox_gpu.py);
  C  epilogue  mean_corr / disc against statmc_prepass of the stored moments and against oracle.prepass, bit for bit.
The starting state is made with numpy and copied in, so it passes through no kernel under test.  Shapes: the smallest at which
each mechanism of the walk can break."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_accumulate_boxcox_cpu import same_bits_or_nan
from test_accumulate_boxcox_gpu import device_box_cox

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5        # BASELINE.json, test_gpu_parity.TOL: where the GPU takes sqrt for pow(x, 0.5)
ALL = ("radiance", "normal", "albedo", "depth", "materialid")
INTERLEAVED = ("materialid", "albedo", "depth", "normal", "radiance")      # the radiance type last, the kinds interleaved
SETS = {
    (0, 1): ("radiance", "depth"),
    (0, 2): ("radiance", "depth", "materialid"),
    (1, 0): ("radiance", "albedo"),
    (1, 1): ("radiance", "normal", "depth"),
    (1, 2): ("radiance", "albedo", "depth", "materialid"),
    (2, 0): ("radiance", "normal", "albedo"),
    (2, 1): ("radiance", "normal", "albedo", "materialid"),
    (2, 2): ALL,
}
# which types are handed over as half (test_accumulate_half_gpu.MIXES)
MIXES = {"fp32": lambda t: False, "features_half": lambda t: t != "radiance", "all_half": lambda t: True,
         "normal_depth_half": lambda t: t in ("normal", "depth")}      # (the last: a mix the fused walk refuses)
FORMATS = ("fp32", "features_half", "all_half")
EVERY = [pytest.param(km, fmt, id="k%dm%d-%s" % (km + (fmt,))) for km in SETS for fmt in FORMATS]
OWN_COUNTS = dict(radiance=5, normal=3, albedo=4, depth=6, materialid=7)
RAGGED_AT = (1, 41)     # 256 x 4: pixel 297, group 74, the second wave of the workgroup
MOMENTS = ("mean", "m2", "m3", "film_mean", "film_m2")


def cfg(t):
    from statmc_amd import film
    return film.STAT_TYPES[t]


def orders(types):
    return (tuple(types), tuple(t for t in INTERLEAVED if t in types))


def planted(W, H):
    """The two poisoned radiance pixels (y, x) and the one far above the rest: on films of four rows and more the first lies in
    row 1 (at 256 pixels a row: the workgroup's second wave), the second in the last row (the film's last wave)."""
    if H >= 4:
        return (1, 5), (H - 1, W - 3), (H // 2, W // 2)
    return (0, 1), (0, W - 1), (0, W // 2)


_SAMPLES, _START, _REF = {}, {}, {}      # this module's samples, starting states and oracle results; emptied by the fixture below
_V, _CHAIN = {}, {}                      # the device's Box-Cox values of the radiance samples, and the oracle's plain chain on them


@pytest.fixture(scope="module", autouse=True)
def shared_inputs():
    """The samples (host and device), starting states and oracle results are computed once and shared by the tests of this module,
    read only; they are released when its last test has run."""
    yield
    for cache in (_SAMPLES, _START, _REF, _V, _CHAIN):
        cache.clear()


def samples(W, H, S, half):
    """({type: [S, H, W, C] fp32 on the host}, the same on the device, the same as half on the device; the last for half only).
    Radiance lognormal(0, 1) with 20 % exact zeros and one x 1000 sample, features uniform in [0, 1); one negative sample (NaN
    through the Box-Cox root) and one huge one in two other pixels.  half: every value rounded to half first, so that both sides
    see the same numbers.  Computed once per shape."""
    key = (W, H, S, half)
    if key not in _SAMPLES:
        from statmc_amd import synthetic
        rng = np.random.default_rng(1000 * W + 10 * H + S)
        host = {}
        for t in ALL:
            c = synthetic.CHANNELS[t]
            if t == "radiance":
                x = rng.lognormal(0, 1, size=(S, H, W, c)).astype(np.float32)
                x[rng.random(x.shape) < 0.2] = 0.0
                a, b, fly = planted(W, H)
                x[S // 2, fly[0], fly[1], 2] = max(float(x[S // 2, fly[0], fly[1], 2]), 0.5) * 1000.0
                if half:
                    x = np.minimum(x, 65504.0).astype(np.float16).astype(np.float32)
                x[0, a[0], a[1], 0] = -1.0
                x[S - 1, b[0], b[1], 1] = 65504.0 if half else 1e6
            else:
                x = rng.random((S, H, W, c), dtype=np.float32)
                if half:
                    x = x.astype(np.float16).astype(np.float32)
            host[t] = x
        wide = {t: torch.from_numpy(x).to(DEV) for t, x in host.items()}
        narrow = {t: x.half() for t, x in wide.items()} if half else None
        if half:
            for t in ALL:
                assert torch.equal(narrow[t].float(), wide[t])
        _SAMPLES[key] = (host, wide, narrow)
        # the device's own Box-Cox value of every radiance sample, read once per sample set (half: through the 16-bit loader)
        from statmc_amd import api
        _V[key] = device_box_cox(api, host["radiance"], "half" if half else "aligned")
    return _SAMPLES[key]


def start_state(W, H, t, count, ragged):
    """One type's starting state on the host (read only): `count` everywhere (ragged: + 2 at RAGGED_AT), random moments where the
    count is positive.  The random planes depend on the film and the type alone."""
    key = (W, H, t, count, ragged)
    if key not in _START:
        c = cfg(t)["channels"]
        rng = np.random.default_rng(77 + 1000 * W + 10 * H + ALL.index(t))
        n = np.full((H, W), count, np.int32)
        if ragged:
            n[RAGGED_AT] += 2
        st = dict(n=n)
        for k in MOMENTS:
            st[k] = (rng.random((H, W, c)) * (n[..., None] > 0)).astype(np.float32)
        if not cfg(t)["transform"]:      # film-mean / film-m2 alias mean / m2 there
            st["film_mean"], st["film_m2"] = st["mean"].copy(), st["m2"].copy()
        _START[key] = st
    return _START[key]


def row_ranges(rows, H):
    if rows is None:
        return ((0, H),)
    return (tuple(rows),) if not hasattr(rows[0], "__len__") else tuple(tuple(r) for r in rows)


def reference(oracle, W, H, S, half, t, count, ragged, rows):
    """oracle.accumulate of one type from its starting state over the rows of the launch (read only, computed once)."""
    key = (W, H, S, half, t, count, ragged, row_ranges(rows, H))
    if key not in _REF:
        smp = samples(W, H, S, half)[0][t]
        ref = {k: v.copy() for k, v in start_state(W, H, t, count, ragged).items()}
        for y0, y1 in row_ranges(rows, H):
            part = {k: np.ascontiguousarray(v[y0:y1]) for k, v in ref.items()}
            oracle.accumulate(part, np.ascontiguousarray(smp[:, y0:y1]), cfg(t)["transform"], cfg(t)["max_moment"])
            for k, v in part.items():
                ref[k][y0:y1] = v
        if t == "radiance":
            # with the oracle alone: the non-finite elements are the planted pixels' (2 pixels x 3 channels at the most)
            a, b, _ = planted(W, H)
            for k in ("mean", "m2", "m3"):
                bad = ~np.isfinite(ref[k])
                assert bad.sum() <= 6, (k, int(bad.sum()))
                bad[a], bad[b] = False, False
                assert not bad.any(), k
            assert np.isfinite(ref["film_mean"]).all() and np.isfinite(ref["film_m2"]).all()
        _REF[key] = ref
    return _REF[key]


def chain(oracle, W, H, S, half, count, ragged, rows):
    """The radiance type's mean / m2 / m3 as the oracle's UNtransformed chain leaves them on the device's own Box-Cox values, from
    the same starting state over the rows of the launch (read only, computed once): the per-element yardstick."""
    key = (W, H, S, half, count, ragged, row_ranges(rows, H))
    if key not in _CHAIN:
        samples(W, H, S, half)
        v = _V[(W, H, S, half)]
        ref = {k: a.copy() for k, a in start_state(W, H, "radiance", count, ragged).items()}
        for y0, y1 in row_ranges(rows, H):
            part = {k: np.ascontiguousarray(a[y0:y1]) for k, a in ref.items()}
            oracle.accumulate(part, np.ascontiguousarray(v[:, y0:y1]), False, 3)
            for k, a in part.items():
                ref[k][y0:y1] = a
        _CHAIN[key] = ref
    return _CHAIN[key]


def new_film(W, H, order, counts, ragged_type, epilogue):
    from statmc_amd import film
    fs = film.FilmStats(W, H, DEV, types=order, fused_prepass=epilogue, g_buffers=())     # (no window filter here: no G-buffers to name)
    for t in order:
        st = start_state(W, H, t, counts[t], t == ragged_type)
        for k, v in fs.state[t].items():
            if v is not None:
                v.copy_(torch.from_numpy(st[k]))
    return fs


@contextlib.contextmanager
def switches(gpu, fused=0, blocks=0):
    try:
        gpu.accumulate_fused(fused)
        gpu.accumulate_resident_blocks(blocks)
        yield
    finally:
        gpu.accumulate_fused(0)
        gpu.accumulate_resident_blocks(0)


def given(W, H, S, order, fmt):
    _, wide, narrow = samples(W, H, S, fmt != "fp32")
    return {t: (narrow[t] if MIXES[fmt](t) else wide[t]) for t in order}, {t: wide[t] for t in order}


def launch_both(gpu, fa, fb, W, H, S, order, fmt, rows=None, blocks=0):
    """The launch under test into fa (the switch at 1), the per-type kernel into fb; returns (fused, loader, grid) of the first
    after asserting that the second did not fuse."""
    lib = gpu.load()
    smp, wide = given(W, H, S, order, fmt)
    with switches(gpu, 1, blocks):
        fa.accumulate(smp, rows=rows)
        got = gpu.last_accumulate_fused(), gpu.last_accumulate_loader(), lib.statmc_debug_last_accumulate_grid()
    with switches(gpu, -1 if fmt == "fp32" else 0):     # half: statmc_accumulate as shipped, which keeps films this small unfused
        fb.accumulate(wide, rows=rows)
        assert gpu.last_accumulate_fused() == 0 and gpu.last_accumulate_loader() == 0
    return got


def bits(x):
    return x.view(torch.int32) if isinstance(x, torch.Tensor) else np.ascontiguousarray(x).view(np.int32)


def assert_same_bits(fa, fb, epilogue, what):
    """A: every plane of every type, NaN payloads included."""
    torch.cuda.synchronize()
    for t in fa.types:
        for k, v in fa.state[t].items():
            if v is not None and not torch.equal(bits(v), bits(fb.state[t][k])):
                diff = (bits(v) != bits(fb.state[t][k])).reshape(-1).nonzero()
                e = int(diff[0])
                c = cfg(t)["channels"] if k != "n" else 1
                raise AssertionError("%s: %s.%s differs from the per-type kernel at %d elements, the first at pixel %d channel %d: %r / %r" % (
                    what, t, k, diff.numel(), e // c, e % c, float(v.reshape(-1)[e]), float(fb.state[t][k].reshape(-1)[e])))
    if epilogue:
        assert torch.equal(bits(fa.mean_corr), bits(fb.mean_corr)), (what, "mean_corr")
        assert torch.equal(bits(fa.disc), bits(fb.disc)), (what, "disc")


def assert_matches_oracle(oracle, fs, W, H, S, half, counts, ragged_type, rows, what):
    """B."""
    for t in fs.types:
        ref = reference(oracle, W, H, S, half, t, counts[t], t == ragged_type, rows)
        got = {k: v.cpu().numpy() for k, v in fs.state[t].items() if v is not None}
        assert np.array_equal(got["n"], ref["n"]), (what, t, "n")
        if t != "radiance":
            assert np.array_equal(bits(got["mean"]), bits(ref["mean"])), (what, t, "mean")
            start = start_state(W, H, t, counts[t], t == ragged_type)
            for k in ("m2", "m3"):                                  # moments above max_moment stay untouched
                assert np.array_equal(bits(got[k]), bits(start[k])), (what, t, k)
            continue
        for k in ("film_mean", "film_m2"):                          # raw-sample moments: exact
            assert np.array_equal(bits(got[k]), bits(ref[k])), (what, t, k)
        for k in ("mean", "m2", "m3"):
            ok = np.isfinite(ref[k])
            assert np.array_equal(np.isfinite(got[k]), ok), (what, t, k, "non-finite elements elsewhere than the oracle's")
            err = rel_l2(got[k][ok], ref[k][ok])
            assert err <= TOL, (what, t, k, err)
        per_element = chain(oracle, W, H, S, half, counts[t], t == ragged_type, rows)
        for k in ("mean", "m2", "m3"):
            same_bits_or_nan(got[k], per_element[k], "%s: radiance.%s against the chain on the device's Box-Cox values" % (what, k))


def assert_epilogue(gpu, oracle, fs, what, spec=None):
    """C: the images the launch's epilogue wrote, against statmc_prepass of the stored moments and the oracle's pre-pass."""
    torch.cuda.synchronize()
    mc, dc = fs.mean_corr.clone(), fs.disc.clone()
    fs._prepass_current = None
    fs.prepass()
    torch.cuda.synchronize()
    assert torch.equal(bits(mc), bits(fs.mean_corr)), (what, "mean_corr / statmc_prepass")
    assert torch.equal(bits(dc), bits(fs.disc)), (what, "disc / statmc_prepass")
    rad = {k: v.cpu().numpy() for k, v in fs.state["radiance"].items()}
    ospec = oracle.default_spec()
    for k, v in (spec or {}).items():
        setattr(ospec, k, v)
    mc_ref, dc_ref = oracle.prepass(rad["n"], rad["mean"], rad["m2"], rad["m3"], spec=ospec)
    assert np.array_equal(mc.cpu().numpy(), mc_ref, equal_nan=True), (what, "mean_corr / oracle")
    assert np.array_equal(dc.cpu().numpy(), dc_ref, equal_nan=True), (what, "disc / oracle")


def run(gpu, oracle, km, fmt, W, H, S, counts=2, epilogue=True, order=0, ragged_type=None, rows=None, blocks=0, fused=1, grid=None,
        spec=None):
    """One launch of set km in format fmt against all three yardsticks."""
    types = orders(SETS[km])[order]
    counts = counts if isinstance(counts, dict) else dict.fromkeys(ALL, counts)
    what = "k%dm%d %s %dx%d S=%d %s counts=%s ragged=%s rows=%s blocks=%d epilogue=%d" % (
        km + (fmt, W, H, S, "/".join(types), [counts[t] for t in types], ragged_type, rows, blocks, epilogue))
    half = fmt != "fp32"
    fa, fb = (new_film(W, H, types, counts, ragged_type, epilogue) for _ in range(2))
    got_fused, got_loader, got_grid = launch_both(gpu, fa, fb, W, H, S, types, fmt, rows, blocks)
    assert got_fused == fused, (what, "fused", got_fused)
    assert got_loader == (1 if half else 0), (what, "loader", got_loader)
    if grid is not None:
        assert got_grid == grid, (what, "grid", got_grid)
    on = epilogue and rows is None
    assert_same_bits(fa, fb, on, what)
    assert_matches_oracle(oracle, fa, W, H, S, half, counts, ragged_type, rows, what)
    if on:
        assert_epilogue(gpu, oracle, fa, what, spec)
    return fa


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("km,fmt", EVERY)
def test_full_waves_batches_around_every_ring_depth(gpu, oracle, km, fmt):
    """256 x 4: one workgroup of four full waves from a uniform count.  The batch lengths are one less than, equal to and one more
    than every ring depth (3 rows fp32, 5 features half, 6 all half) and 3 D + 1 for each."""
    for S in (1, 2, 3, 4, 5, 6, 7, 8, 13, 19):
        for order in (0, 1):
            run(gpu, oracle, km, fmt, 256, 4, S, order=order, grid=1)


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("km,fmt", EVERY)
def test_partial_and_tiny_waves(gpu, oracle, km, fmt):
    """248 x 5: 310 groups, the last wave of 54 lanes -- fp32 keeps it in the counted-transfer walk (the pieces beyond the row's end
    re-read its start), half hands it to accumulate_fused_ragged beside fused waves.  8 x 1: two lanes.  fp32 alone (1260 and 4
    pixels are no multiple of 8): 252 x 5, 59 lanes, and 4 x 1, the smallest eligible film, one lane."""
    shapes = [(248, 5, 2), (8, 1, 1)] + ([(252, 5, 2), (4, 1, 1)] if fmt == "fp32" else [])
    for W, H, grid in shapes:
        for epilogue in (True, False):
            for order in (0, 1):
                run(gpu, oracle, km, fmt, W, H, 7, epilogue=epilogue, order=order, grid=grid)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("km,fmt", EVERY)
def test_grid_stride_passes(gpu, oracle, km, fmt):
    """512 x 6: three 256-group units on one workgroup, then on two (one makes two passes).  Seven samples: a pass ends on a ring
    slot other than 0 at every depth, and the next one starts the ring and the counted waits again."""
    for blocks in (1, 2):
        for order in (0, 1):
            run(gpu, oracle, km, fmt, 512, 6, 7, order=order, blocks=blocks, grid=blocks)


# ------------------------------------------------------------------ 4
def count_tables(km):
    """Every type from its own count, and the same with the counts of the two types of a kind swapped."""
    tables = [OWN_COUNTS]
    if km[0] == 2:
        tables.append(dict(OWN_COUNTS, normal=OWN_COUNTS["albedo"], albedo=OWN_COUNTS["normal"]))
    if km[1] == 2:
        tables.append(dict(OWN_COUNTS, depth=OWN_COUNTS["materialid"], materialid=OWN_COUNTS["depth"]))
    return tables


@pytest.mark.parametrize("km,fmt", EVERY)
def test_every_type_from_its_own_count(gpu, oracle, km, fmt):
    """Counts uniform within a type and different in every type: one reciprocal per type and sample (walk(std::false_type)).  A
    count taken from another type's changes that type's means, which the per-type kernel and the oracle do not follow."""
    for counts in count_tables(km):
        for order in (0, 1):
            run(gpu, oracle, km, fmt, 256, 4, 7, counts=counts, order=order, grid=1)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("km,fmt", EVERY)
def test_ragged_counts_in_every_type_in_turn(gpu, oracle, km, fmt):
    """One pixel of the second wave has seen two samples more in ONE type: that wave takes accumulate_fused_ragged, which names
    its descriptors by position (the second type of a kind too), the waves beside it stay on the fused walk, and the launch
    reports itself fused."""
    for ragged_type in SETS[km]:
        for order in (0, 1):
            run(gpu, oracle, km, fmt, 256, 4, 7, counts=OWN_COUNTS, order=order, ragged_type=ragged_type, grid=1)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("km,fmt", EVERY)
def test_row_ranges(gpu, oracle, km, fmt):
    """256 x 4, rows 1 .. 2 (n_elems < stride: what the multi-GPU step launches once the border rows are split off): fused, the
    rows outside keep every bit, and through the C ABI the epilogue writes those rows only.  Two ranges in one launch carry every
    type twice and keep the per-type kernel."""
    W, H, S = 256, 4, 7
    lib = gpu.load()
    half = fmt != "fp32"
    for order in (0, 1):
        types = orders(SETS[km])[order]
        fa = run(gpu, oracle, km, fmt, W, H, S, order=order, rows=(1, 3), grid=1)
        torch.cuda.synchronize()
        for t in types:
            start = start_state(W, H, t, 2, False)
            for k, v in fa.state[t].items():
                if v is not None:
                    for y in (0, 3):
                        assert np.array_equal(bits(v[y].cpu().numpy()), bits(start[k][y])), (types, t, k, y)
            assert int(fa.state[t]["n"][1:3].min()) == 2 + S
        # the same launch with the radiance type's epilogue, on images filled beforehand
        fc = new_film(W, H, types, dict.fromkeys(ALL, 2), None, False)
        mc, dc = torch.full_like(fc.mean_corr, 3.0), torch.full_like(fc.disc, 3.0)
        smp, _ = given(W, H, S, types, fmt)
        sts = [gpu.make_stat_type(smp[t], fc.state[t], cfg(t)["transform"], cfg(t)["max_moment"], prepass_into=(mc, dc) if t == "radiance" else None)
               for t in types]
        fmts = [gpu.SAMPLES_F16 if smp[t].dtype == torch.float16 else gpu.SAMPLES_F32 for t in types]
        with switches(gpu, 1):
            gpu.accumulate(W, H, sts, rows=(1, 3), sample_formats=fmts if half else None)
            assert gpu.last_accumulate_fused() == 1 and lib.statmc_debug_last_accumulate_grid() == 1, (types, "epilogue over a row range")
        assert_same_bits(fc, fa, False, "%s rows (1, 3) with the epilogue against without" % (types,))
        fc.prepass()
        torch.cuda.synchronize()
        assert torch.equal(bits(mc[1:3]), bits(fc.mean_corr[1:3])) and torch.equal(bits(dc[1:3]), bits(fc.disc[1:3])), types
        three = torch.full_like(mc[0], 3.0)
        for y in (0, 3):
            assert torch.equal(bits(mc[y]), bits(three)) and torch.equal(bits(dc[y]), bits(three)), (types, y)
        run(gpu, oracle, km, fmt, W, H, S, order=order, rows=[(0, 1), (2, 4)], fused=0)


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("spec", [dict(sides=1, small_n=1), dict(dof=1)], ids=["two-sided-exclude", "welch"])
@pytest.mark.parametrize("km,fmt", [pytest.param(km, fmt, id="k%dm%d-%s" % (km + (fmt,))) for km in ((0, 1), (2, 2)) for fmt in ("fp32", "all_half")])
def test_epilogue_under_the_specs_that_change_it(gpu, oracle, km, fmt, spec):
    """The fused walk's own epilogue under the quantile sides / n < 2 exclusion and Welch's degrees of freedom: from a zero state
    with one sample (n = 1 everywhere) and from count 2 with four."""
    gpu.set_filter_spec(**spec)
    try:
        for counts, S in ((0, 1), (2, 4)):
            for order in (0, 1):
                run(gpu, oracle, km, fmt, 256, 4, S, counts=counts, order=order, grid=1, spec=spec)
    finally:
        gpu.set_filter_spec()


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("W,H", [(256, 4), (248, 5)])
def test_a_mix_that_must_not_fuse(gpu, oracle, W, H):
    """All five types with only `normal` and `depth` half: a feature type in fp32 beside half ones keeps the per-type 16-bit kernel
    (vector loader), with the switch at 1 too."""
    for order in (0, 1):
        run(gpu, oracle, (2, 2), "normal_depth_half", W, H, 7, order=order, fused=0)
