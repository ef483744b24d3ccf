"""statmc_compact_accumulate on the GPU: a compact arena -- every pixel's samples back to back, pixels in raster order -- leaves,
per pixel, the bits statmc_accumulate_records leaves for the same samples in the same order (statmc_accumulate_records_split above
split_above), whatever kernel folds it.  Every case runs under the default dispatch, under the forced staged kernel and under the
forced direct kernel, and statmc_debug_last_compact_path says which KERNEL it held to the definition.  Inside the staged kernel a
wave stages only where its 64 pixels' span fits 12 KiB, no run is above split_above and the runs tile the span; the other waves take
the direct fold in that kernel.  So under "staged" the uniform-16, 0 .. 9, odd-halfword and front-skew cases run the LDS path, while
the wave at 300 samples, the split pixels' waves and the waves around wrong offsets are held to the in-kernel direct fold, next to
staging neighbours.  Comparisons are bitwise on int32 views of every state image unless a test says otherwise."""
import subprocess

import numpy as np
import pytest

import compact_reference as ref
from test_records_gpu import (FIELDS, FILMS, KINDS, TYPES, States, assert_matches_the_oracle, bits, dev, make_samples, ragged_counts,
                              run_arena, same)

pytestmark = pytest.mark.gpu

INT32_MAX = ref.INT32_MAX
PATHS = ("auto", "staged", "direct")


def as_half(samples):
    """[n, C] fp32 -> fp16 arenas (the firefly kept finite) and the fp32 values the fold sees"""
    h = [np.clip(s, 0, 60000).astype(np.float16) for s in samples]
    return h, [x.astype(np.float32) for x in h]


def junk(rng, n, dtype, finite=False):
    """n guard elements: NaN, +inf, -inf and the format's largest numbers; finite: large finite junk only"""
    big = np.finfo(dtype).max
    pool = np.array([big, -big, 12345.0, -777.0] if finite else [np.nan, np.inf, -np.inf, big, -big], dtype=dtype)
    return pool[rng.integers(0, pool.size, n)]


def run_compact(api, S, offsets, samples, n_samples=None, split_above=INT32_MAX, path="auto", front=0, back=0, guard_rng=None, finite_guards=False,
                d_offsets=None):
    """One statmc_compact_accumulate call into S.  samples: per type [n, C] in fp32 or fp16 (the type's format); front / back: guard
    ELEMENTS in front of every arena and behind its n_samples samples.  Returns what statmc_debug_last_compact_path reports."""
    import torch
    n_samples = samples[0].shape[0] if n_samples is None else n_samples
    rng = guard_rng if guard_rng is not None else np.random.default_rng(0)
    keep, sts, fmts = [], [], []
    for i, k in enumerate(S.types):
        s = samples[i].reshape(-1)
        assert s.size == n_samples * k[1]
        whole = dev(np.concatenate([junk(rng, front, s.dtype, finite_guards), s, junk(rng, back, s.dtype, finite_guards)]))
        keep.append(whole)
        arena = whole[front:front + s.size] if s.size else whole[front:front]
        sts.append(api.make_stat_type_compact(arena, k[1], S.st[i], k[2], k[3], prepass_into=S.pre(i)))
        fmts.append(api.SAMPLES_F16 if s.dtype == np.float16 else api.SAMPLES_F32)
    d_off = d_offsets if d_offsets is not None else dev(np.asarray(offsets, np.int64))
    api.compact_path({"auto": api.COMPACT_PATH_AUTO, "staged": api.COMPACT_PATH_STAGED, "direct": api.COMPACT_PATH_DIRECT}[path])
    try:
        api.compact_accumulate(S.W, S.H, sts, d_off, n_samples=n_samples, sample_formats=fmts if api.SAMPLES_F16 in fmts else None, split_above=split_above)
    finally:
        api.compact_path(api.COMPACT_PATH_AUTO)
    torch.cuda.synchronize()
    return api.last_compact_path()


def assert_path(api, got, path, split_above):
    kernel, split = got & ~api.COMPACT_PATH_SPLIT, got & api.COMPACT_PATH_SPLIT
    if path == "auto":
        assert kernel in (api.COMPACT_PATH_STAGED, api.COMPACT_PATH_DIRECT), got
    else:
        assert kernel == (api.COMPACT_PATH_STAGED if path == "staged" else api.COMPACT_PATH_DIRECT), (path, got)
    assert bool(split) == (split_above != INT32_MAX), (got, split_above)


def run_records(api, S, pixels, samples, split_above=None):
    """the yardstick: statmc_accumulate_records[_split] on fp32 record arrays"""
    import torch
    d_px = dev(np.asarray(pixels, np.int32))
    d_s = [dev(np.ascontiguousarray(s, np.float32)) for s in samples]
    sts = [api.make_stat_type_records(d_s[i], k[1], S.st[i], k[2], k[3], prepass_into=S.pre(i)) for i, k in enumerate(S.types)]
    api.accumulate_records(S.W, S.H, sts, d_px, split_above=split_above)
    torch.cuda.synchronize()


def hold_to_the_records_entry(api, W, H, counts, samples, types=TYPES, widened=None, split_above=INT32_MAX, fill_seed=None, **kw):
    """counts [W * H], samples per type [total, C] (fp32, or fp16 with `widened` the fp32 values): on every path the compact call
    equals the records entry on (owners, samples).  fill_seed: both sides continue the state two earlier samples per pixel left
    (the records entry's), so the folds start from counts, moments and an epilogue that are not zero.  Returns that result."""
    counts = np.asarray(counts, np.int64)
    offsets = ref.offsets_ref(counts)
    owners = ref.owners_ref(counts, int(offsets[-1]))

    def fresh():
        S = States(W, H, types=types)
        if fill_seed is not None:
            run_records(api, S, np.repeat(np.arange(W * H, dtype=np.int32), 2), make_samples(np.random.default_rng(fill_seed), 2 * W * H, types))
        return S
    B = fresh()
    run_records(api, B, owners, widened if widened is not None else samples, split_above=None if split_above == INT32_MAX else split_above)
    want = B.snapshot()
    for path in PATHS:
        A = fresh()
        assert_path(api, run_compact(api, A, offsets, samples, split_above=split_above, path=path, **kw), path, split_above)
        same(A.snapshot(), want)
    return want


# ---------------------------------------------------------------- equality with the records entry, the dense arena and the oracle
@pytest.fixture(scope="module", params=FILMS, ids=lambda f: "%dx%d" % f)
def ragged(request, gpu):
    """One ragged compact arena per film, laid out by statmc_compact_offsets itself, and the records entry's result on its owners."""
    import torch
    W, H = request.param
    rng = np.random.default_rng(2000 + W)
    counts = ragged_counts(rng, W * H)
    total = int(counts.sum())
    d_offsets, d_owners = gpu.compact_offsets(dev(counts.astype(np.int32).reshape(H, W)), owners_capacity=total)
    torch.cuda.synchronize()
    offsets, owners = d_offsets.cpu().numpy(), d_owners.cpu().numpy()
    assert int(offsets[-1]) == total
    samples = make_samples(rng, total)
    B = States(W, H)
    run_records(gpu, B, owners, samples)
    return W, H, counts, offsets, owners, samples, B.snapshot()


@pytest.mark.parametrize("path", PATHS)
def test_ragged_counts_equal_the_records_entry(gpu, ragged, path):
    W, H, counts, offsets, owners, samples, want = ragged
    assert (counts == 0).mean() > 0.1 and counts.max() == 300
    A = States(W, H)
    assert_path(gpu, run_compact(gpu, A, offsets, samples, path=path), path, INT32_MAX)
    assert np.array_equal(A.st[0]["n"].cpu().numpy().reshape(-1), counts)
    same(A.snapshot(), want)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
def test_uniform_counts_equal_the_records_entry_and_the_dense_arena(gpu, film):
    W, H = film
    rng = np.random.default_rng(17 + W)
    counts = np.full(W * H, 16)
    samples = make_samples(rng, int(counts.sum()))
    want = hold_to_the_records_entry(gpu, W, H, counts, samples)
    D = States(W, H)
    run_arena(gpu, D, ref.owners_ref(counts, int(counts.sum())), samples, 16)      # statmc_accumulate on the transposed dense arena
    same(D.snapshot(), want)


@pytest.mark.parametrize("path", PATHS)
def test_ragged_counts_match_the_oracle(gpu, oracle, ragged, path):
    W, H, counts, offsets, owners, samples, _ = ragged
    S = States(W, H)
    run_compact(gpu, S, offsets, samples, path=path)
    assert_matches_the_oracle(oracle, S, counts, owners, samples)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_every_body_of_the_type_dispatch(gpu, half):
    """The twelve (channels, transform, max_moment) kinds in one call, on runs at every edge of the walks: empty, shorter than a
    batch of four, whole batches in odd and even number, each with and without a tail."""
    W, H = FILMS[0]
    rng = np.random.default_rng(41)
    counts = np.resize(np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17]), W * H)
    samples = make_samples(rng, int(counts.sum()), KINDS)
    if half:
        samples, widened = as_half(samples)
        hold_to_the_records_entry(gpu, W, H, counts, samples, types=KINDS, widened=widened)
    else:
        hold_to_the_records_entry(gpu, W, H, counts, samples, types=KINDS)


# ---------------------------------------------------------------- ring and span edges on 64 x 32
def edge_counts(name):
    W, H = 64, 32
    rng = np.random.default_rng(sum(map(ord, name)))
    c = rng.integers(0, 10, W * H).astype(np.int64)
    if name == "a_whole_wave_at_300":           # 64 consecutive pixels, one wave: 230 KB of RGB fp32 in one span
        c[64:128] = 300
    elif name == "a_wave_with_nothing":
        c[128:192] = 0
    elif name == "a_workgroup_with_nothing":
        c[256:512] = 0
    elif name == "one_pixel_at_300_among_zeros":
        c[:] = 0
        c[777] = 300
    elif name == "only_the_last_pixel":
        c[:] = 0
        c[-1] = 5
    return W, H, c


@pytest.mark.parametrize("name", ["a_whole_wave_at_300", "a_wave_with_nothing", "a_workgroup_with_nothing", "one_pixel_at_300_among_zeros",
                                  "only_the_last_pixel"])
def test_span_edges(gpu, name):
    W, H, counts = edge_counts(name)
    samples = make_samples(np.random.default_rng(5), int(counts.sum()))
    want = hold_to_the_records_entry(gpu, W, H, counts, samples, fill_seed=9)
    assert want[0].reshape(-1).size == W * H


def test_arenas_that_start_four_bytes_into_their_allocation(gpu):
    W, H = 64, 32
    rng = np.random.default_rng(77)
    counts = rng.integers(0, 10, W * H)
    samples = make_samples(rng, int(counts.sum()))
    for front in (1, 2, 3):       # every 4-byte phase of the 16-byte staging piece
        hold_to_the_records_entry(gpu, W, H, counts, samples, front=front, back=5, guard_rng=np.random.default_rng(front))


def test_a_one_channel_half_arena_whose_runs_start_at_odd_halfwords(gpu):
    W, H = 64, 32
    rng = np.random.default_rng(78)
    counts = 2 * rng.integers(0, 6, W * H) + 1          # odd counts: every second run starts at an odd halfword
    counts[rng.random(W * H) < 0.1] = 0
    depth = [TYPES[2], TYPES[3]]                          # the 1-channel types
    samples, widened = as_half(make_samples(rng, int(counts.sum()), depth))
    for front in (0, 1, 3):       # ... and with an odd front, the others
        hold_to_the_records_entry(gpu, W, H, counts, samples, types=depth, widened=widened, front=front, back=3, guard_rng=np.random.default_rng(front))


def test_a_three_pixel_film(gpu):
    rng = np.random.default_rng(79)
    for counts in ([2, 0, 5], [0, 0, 1], [70, 3, 0]):
        samples = make_samples(rng, sum(counts))
        hold_to_the_records_entry(gpu, 3, 1, np.array(counts), samples)


# ---------------------------------------------------------------- split
def test_runs_above_split_above_equal_the_split_records_entry(gpu):
    W, H = 64, 32
    rng = np.random.default_rng(80)
    counts = rng.integers(0, 10, W * H)
    counts[710], counts[713], counts[1500] = 300, 33, 32      # two split pixels in one wave, with short neighbours; 32 is not above 32
    samples = make_samples(rng, int(counts.sum()))
    split = hold_to_the_records_entry(gpu, W, H, counts, samples, split_above=32)
    sequential = hold_to_the_records_entry(gpu, W, H, counts, samples, split_above=300)        # nothing is above 300: the sequential bits
    B = States(W, H)
    run_records(gpu, B, ref.owners_ref(counts, int(counts.sum())), samples)
    same(sequential, B.snapshot())
    differs = [int((a.reshape(W * H, -1) != b.reshape(W * H, -1)).any(axis=1).sum()) for a, b in zip(split, sequential)]
    assert max(differs) <= 2      # the two split pixels alone may hold other last bits


# ---------------------------------------------------------------- nothing outside the runs reaches a state
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_guard_bands_of_nan_and_inf_change_nothing(gpu, ragged, half):
    """NaN / inf / largest-finite values in front of the arena, behind n_samples, and inside it behind offsets[W * H] (n_samples
    larger than the total)."""
    W, H, counts, offsets, owners, samples, want = ragged
    slack = 40
    total = int(offsets[-1])
    if half:
        samples, widened = as_half(samples)
        B = States(W, H)
        run_records(gpu, B, owners, widened)
        want = B.snapshot()
    rng = np.random.default_rng(31)
    padded = [np.concatenate([s, junk(rng, slack * s.shape[1], s.dtype).reshape(slack, -1)]) for s in samples]
    for path in PATHS:
        A = States(W, H)
        run_compact(gpu, A, offsets, padded, n_samples=total + slack, path=path, front=64, back=64, guard_rng=np.random.default_rng(32))
        same(A.snapshot(), want)


def test_wrong_offsets_stay_inside_the_arena(gpu, ragged):
    """A negative entry, a decreasing pair and an entry beyond n_samples are clamped BEFORE they become an address.  The arenas carry
    guard bands of finite junk on both sides, longer than the largest wrong offset: a kernel that clamps late reads memory that
    exists and fails by its bits.  Expected: the records entry on the clamped runs."""
    W, H, counts, offsets, owners, samples, _ = ragged
    total = int(offsets[-1])
    wrong = offsets.copy()
    wrong[10] = -50
    wrong[200] = wrong[199] - 30
    wrong[500] = total + 1000
    start, end = ref.clamp_runs(wrong, total)
    assert (start > end).sum() == 0 and (np.diff(wrong) < 0).any() and wrong.min() < 0 and wrong.max() > total
    pixels, positions = ref.records_of_runs(start, end)
    B = States(W, H)
    run_records(gpu, B, pixels, [s[positions] for s in samples])
    want = B.snapshot()
    guard = 1100 * 3      # elements: more than 1000 samples of the widest type on either side
    for path in PATHS:
        A = States(W, H)
        run_compact(gpu, A, wrong, samples, path=path, front=guard, back=guard, guard_rng=np.random.default_rng(33), finite_guards=True)
        same(A.snapshot(), want)


def test_untouched_pixels_keep_every_bit(gpu, ragged):
    W, H, counts, offsets, owners, samples, _ = ragged
    for path in PATHS:
        S = States(W, H, fill=np.random.default_rng(5))
        for st in S.st:
            st["n"].remainder_(1000).abs_()
        before = S.snapshot()
        run_compact(gpu, S, offsets, samples, path=path)
        after = S.snapshot()
        untouched = counts == 0
        assert untouched.any()
        for x, y in zip(before, after):       # every image, mean_corr / discriminator included
            assert np.array_equal(x.reshape(W * H, -1)[untouched], y.reshape(W * H, -1)[untouched])
        assert np.array_equal(after[0].reshape(-1) - before[0].reshape(-1), counts)
        # an arena of no samples and a call without types: nothing changes anywhere
        run_compact(gpu, S, np.zeros(W * H + 1, np.int64), [s[:0] for s in samples], path=path)
        assert gpu.last_compact_path() == 0
        same(after, S.snapshot())
    import torch
    gpu.compact_accumulate(W, H, [], dev(offsets), n_samples=int(offsets[-1]))
    torch.cuda.synchronize()
    assert gpu.last_compact_path() == 0
    same(after, S.snapshot())


def test_two_calls_equal_one(gpu, ragged):
    """[the first k samples of every run], then [the rest] with rebased offsets, equals one call when nothing is split."""
    W, H, counts, offsets, owners, samples, want = ragged
    k = 3
    start = offsets[:-1]
    head = np.minimum(counts, k)
    for path in PATHS:
        S = States(W, H)
        for lo, hi in ((start, start + head), (start + head, start + counts)):
            _, positions = ref.records_of_runs(lo, hi)
            run_compact(gpu, S, ref.offsets_ref(hi - lo), [s[positions] for s in samples], path=path)
        same(S.snapshot(), want)


def test_three_runs_give_the_same_bits(gpu, ragged):
    W, H, counts, offsets, owners, samples, want = ragged
    for path in PATHS:
        for run in range(3):
            S = States(W, H)
            run_compact(gpu, S, offsets, samples, split_above=64, path=path)
            if run == 0:
                first = S.snapshot()
            else:
                same(first, S.snapshot())


def test_on_a_side_stream(gpu, ragged):
    """On a statmc_stream_create side stream while torch's current stream is the null stream; the inputs are copied in on that side
    stream just before the call.  Equals the null-stream result."""
    import ctypes as C
    import torch
    api, lib = gpu, gpu.load()
    W, H, counts, offsets, owners, samples, want = ragged
    assert torch.cuda.current_stream().cuda_stream == 0
    # torch never hears of the side stream: its tensors are allocated and zeroed on the null stream, which is then drained, and
    # the library's own upload fills them on the side stream
    host = [np.ascontiguousarray(s) for s in samples] + [np.ascontiguousarray(offsets)]
    side = C.c_void_p()
    api.check(lib.statmc_stream_create(C.byref(side)))
    try:
        for path in PATHS:
            S = States(W, H)
            d = [torch.zeros(h.shape, dtype=torch.from_numpy(h).dtype, device="cuda:0") for h in host]
            torch.cuda.synchronize()
            for dst, src in zip(d, host):
                api.check(lib.statmc_upload(dst.data_ptr(), src.ctypes.data, src.nbytes, side))
            sts = [api.make_stat_type_compact(d[i], k[1], S.st[i], k[2], k[3], prepass_into=S.pre(i)) for i, k in enumerate(S.types)]
            api.compact_path({"auto": 0, "staged": api.COMPACT_PATH_STAGED, "direct": api.COMPACT_PATH_DIRECT}[path])
            try:
                api.compact_accumulate(W, H, sts, d[-1], split_above=INT32_MAX, stream=side)
            finally:
                api.compact_path(0)
            api.check(lib.statmc_synchronize(side))
            same(S.snapshot(), want)
    finally:
        api.check(lib.statmc_synchronize(side))
        api.check(lib.statmc_stream_destroy(side))


# ---------------------------------------------------------------- the wrappers
def test_filmstats_accumulate_compact_with_half_features(gpu):
    import torch
    from statmc_amd import film
    api = gpu
    W, H = FILMS[0]
    rng = np.random.default_rng(90)
    counts = ragged_counts(rng, W * H)
    total = int(counts.sum())
    names = ("radiance", "normal", "albedo")
    host = {"radiance": make_samples(rng, total, [TYPES[0]])[0], "normal": rng.random((total, 3)).astype(np.float16),
            "albedo": rng.random((total, 3)).astype(np.float16)}
    d = {k: dev(v) for k, v in host.items()}
    offsets, _ = api.compact_offsets(dev(counts.astype(np.int32).reshape(H, W)))
    fs = film.FilmStats(W, H, torch.device("cuda:0"), types=names)
    fs.accumulate_compact(d, offsets)
    assert api.last_compact_path() & api.COMPACT_PATH_SPLIT      # the wrapper's default: STATMC_RECORDS_SPLIT_DEFAULT
    st = {t: film.new_state(H, W, 3, torch.device("cuda:0"), transform=film.STAT_TYPES[t]["transform"]) for t in names}
    sts = [api.make_stat_type_compact(d[t], 3, st[t], film.STAT_TYPES[t]["transform"], film.STAT_TYPES[t]["max_moment"]) for t in names]
    api.compact_accumulate(W, H, sts, offsets, sample_formats=[api.SAMPLES_F32, api.SAMPLES_F16, api.SAMPLES_F16])
    torch.cuda.synchronize()
    for t in names:
        for k in FIELDS:
            if st[t].get(k) is not None:
                assert np.array_equal(bits(fs.state[t][k]), bits(st[t][k])), (t, k)
    assert np.array_equal(fs.state["normal"]["n"].cpu().numpy().reshape(-1), counts)
    with pytest.raises(TypeError):
        fs.accumulate_compact({"radiance": d["radiance"].double()}, offsets)


def test_estimator_plan_offsets_accumulate_compact_equals_accumulate_records(gpu):
    """Estimator::PlanSamples -> CompactOffsets -> AccumulateCompact on one stream against AccumulateRecords on the owners
    (tests/cpp/test_compact_accumulate.cpp)."""
    from statmc_amd import build
    build.build_tools()
    for w, h in ((61, 37), (96, 64)):
        out = subprocess.run([build.COMPACT_BIN, str(w), str(h)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "compact accumulate ok" in out.stdout
