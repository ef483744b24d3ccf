"""statmc_compact_accumulate_interleaved on the GPU: a compact arena of interleaved records -- pixel p's records at slots
[offsets[p], offsets[p + 1]) of ONE array -- leaves, per pixel, the bits statmc_compact_accumulate leaves on the de-interleaved
arenas, hence those of the records entries on the same samples, whatever kernel folds it.  Every case runs under the default
dispatch and under each forced kernel that applies (fused staged, fused direct, general), and
statmc_debug_last_compact_interleaved_path says which KERNEL it held to the definition.  Inside the staged kernel a wave stages
only where the span of its 64 pixels fits the LDS window, no run is above split_above and the runs tile the span; the other waves
fold directly in that kernel.  Comparisons are bitwise on int32 views of every state image."""
import subprocess

import numpy as np
import pytest

import compact_reference as ref
import test_records_gpu as arrays_tests
from test_records_interleaved_gpu import F16, F32, FILMS, FIVE, FOUR, bits, dev, make_fields, ragged_counts
from test_records_interleaved_gpu import States as FilledStates

pytestmark = pytest.mark.gpu

INT32_MAX = ref.INT32_MAX
KINDS = arrays_tests.KINDS
BATCH = 4                      # kCompactBatch: records per request group of the walks
PATHS = ("auto", "staged", "direct", "general")
OFFSETS = {"five": (0, 12, 24, 36, 40), "four": (0, 12, 24, 28)}      # fp32 fields of the two sets in a 44- or 48-byte record
SETS = {"five": FIVE, "four": FOUR}


def States(W, H, kinds, fill=False):
    """Zeroed state images: a fold that starts from what real samples left is a case of its own (the continued state below).  The
    records tests' random bit patterns hold NaNs, and two kernels that add the same two NaNs in another operand order keep another
    payload: no bits any definition promises."""
    return FilledStates(W, H, kinds, fill=fill)


def same(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if not np.array_equal(x, y):
            at = np.flatnonzero(x.reshape(-1) != y.reshape(-1))
            raise AssertionError("%s: image %d differs in %d elements, first at %d: %#x against %#x" % (
                what, k, at.size, at[0], int(x.reshape(-1)[at[0]]) & 0xffffffff, int(y.reshape(-1)[at[0]]) & 0xffffffff))


def pack(fields, offsets, stride, formats=None, fill=0xEE, owners=None, pixel_offset=None):
    """[n, C] arrays -> uint8 [n * stride]: field i at offsets[i] in its format (a half field is rounded to IEEE half here), later
    fields winning where fields overlap, `fill` everywhere else; owners: int32 written at pixel_offset last."""
    n = fields[0].shape[0]
    formats = [F32] * len(fields) if formats is None else formats
    rec = np.full((n, stride), fill, dtype=np.uint8)
    for f, o, fmt in zip(fields, offsets, formats):
        a = np.ascontiguousarray(f, dtype=np.float16 if fmt == F16 else np.float32)
        b = a.view(np.uint8).reshape(n, f.shape[1] * a.itemsize)
        assert o + b.shape[1] <= stride
        rec[:, o:o + b.shape[1]] = b
    if owners is not None:
        rec[:, pixel_offset:pixel_offset + 4] = np.ascontiguousarray(owners, dtype=np.int32).view(np.uint8).reshape(n, 4)
    return rec.reshape(-1)


def in_format(fields, formats):
    """the de-interleaved arenas, each in its field's format"""
    if formats is None:
        return fields
    return [f.astype(np.float16) if fmt == F16 else f for f, fmt in zip(fields, formats)]


def field_types(api, S):
    return [api.make_stat_type_record_field(k[1], S.st[i], k[2], k[3], prepass_into=S.pre_images[i]) for i, k in enumerate(S.kinds)]


def run_ilv(api, S, rec, stride, field_offsets, offsets, formats=None, n_records=None, split_above=INT32_MAX, path="auto", front=0, back=0,
            pixel_offset=0, stream=None):
    """One statmc_compact_accumulate_interleaved call into S.  front / back: guard BYTES (0xFF: NaN in either format) in front of
    the records and behind them.  Returns what statmc_debug_last_compact_interleaved_path reports."""
    import torch
    n_records = rec.size // stride if n_records is None else n_records
    whole = dev(np.concatenate([np.full(front, 0xFF, np.uint8), rec, np.full(back, 0xFF, np.uint8)]))
    d_rec = whole[front:front + rec.size]
    assert d_rec.data_ptr() % 16 == front % 16
    layout = api.make_record_layout(stride, pixel_offset, field_offsets, formats)
    d_off = dev(np.asarray(offsets, np.int64))
    api.compact_interleaved_path(PATHS.index(path))
    try:
        api.compact_accumulate_interleaved(S.W, S.H, field_types(api, S), d_rec, layout, d_off, n_records=n_records, split_above=split_above, stream=stream)
        torch.cuda.synchronize()
    finally:
        api.compact_interleaved_path(0)
    return api.last_compact_interleaved_path()


def assert_path(api, got, path, fusable, split_above):
    kernel, split = got & 3, got & api.COMPACT_ILV_PATH_SPLIT
    fused = (api.COMPACT_ILV_PATH_FUSED_STAGED, api.COMPACT_ILV_PATH_FUSED_DIRECT)
    if not fusable or path == "general":
        assert kernel == api.COMPACT_ILV_PATH_GENERAL, (path, got)
    elif path == "auto":
        assert kernel in fused, got
    else:
        assert kernel == fused[path == "direct"], (path, got)
    assert bool(split) == (split_above != INT32_MAX), (got, split_above)


def paths_of(fusable):
    return PATHS if fusable else ("auto", "general")


def run_compact_arrays(api, S, offsets, arenas, split_above=INT32_MAX):
    """yardstick 1: statmc_compact_accumulate on one arena per type, each in its field's format"""
    import torch
    d = [dev(a) for a in arenas]
    sts = [api.make_stat_type_compact(d[i], k[1], S.st[i], k[2], k[3], prepass_into=S.pre_images[i]) for i, k in enumerate(S.kinds)]
    fmts = [F16 if a.dtype == np.float16 else F32 for a in arenas]
    api.compact_accumulate(S.W, S.H, sts, dev(np.asarray(offsets, np.int64)), n_samples=arenas[0].shape[0], sample_formats=fmts if F16 in fmts else None,
                           split_above=split_above)
    torch.cuda.synchronize()


def run_records_ilv(api, S, rec, stride, field_offsets, pixel_offset, formats=None, split_above=None):
    """yardstick 2: statmc_accumulate_records_interleaved[_split] on records that carry their owner in a pixel field"""
    import torch
    layout = api.make_record_layout(stride, pixel_offset, field_offsets, formats)
    api.accumulate_records_interleaved(S.W, S.H, field_types(api, S), dev(rec), layout, n_records=rec.size // stride, split_above=split_above)
    torch.cuda.synchronize()


def run_records_arrays(api, S, pixels, fields, split_above=None):
    """yardstick 3: statmc_accumulate_records[_split] on fp32 arrays"""
    import torch
    d_px = dev(np.asarray(pixels, np.int32))
    d_s = [dev(np.ascontiguousarray(f, np.float32)) for f in fields]
    sts = [api.make_stat_type_records(d_s[i], k[1], S.st[i], k[2], k[3], prepass_into=S.pre_images[i]) for i, k in enumerate(S.kinds)]
    api.accumulate_records(S.W, S.H, sts, d_px, split_above=split_above)
    torch.cuda.synchronize()


def hold_to_the_compact_entry(api, W, H, kinds, counts, fields, field_offsets, stride, formats=None, fusable=False, split_above=INT32_MAX,
                              offsets=None, **kw):
    """On every path that applies the new entry on the packed records equals statmc_compact_accumulate on the de-interleaved
    arenas (same offsets, same split_above, every arena in its field's format).  Returns that result."""
    offsets = ref.offsets_ref(np.asarray(counts, np.int64)) if offsets is None else offsets
    B = States(W, H, kinds)
    run_compact_arrays(api, B, offsets, in_format(fields, formats), split_above=split_above)
    want = B.snapshot()
    rec = pack(fields, field_offsets, stride, formats)
    for path in paths_of(fusable):
        A = States(W, H, kinds)
        got = run_ilv(api, A, rec, stride, field_offsets, offsets, formats=formats, split_above=split_above, path=path, **kw)
        if rec.size:
            assert_path(api, got, path, fusable, split_above)
        same(want, A.snapshot(), "path %s" % path)
    return want


# ---------------------------------------------------------------- ragged counts: both yardsticks, both strides, both type sets
@pytest.fixture(scope="module", params=[(f, s) for f in FILMS for s in SETS], ids=lambda p: "%dx%d-%s" % (p[0][0], p[0][1], p[1]))
def ragged(request, gpu):
    """One ragged compact arena per film and type set, and what the two yardsticks leave for it: statmc_compact_accumulate on the
    de-interleaved arenas, statmc_accumulate_records_interleaved on the 48-byte records with the owners at byte 44."""
    (W, H), name = request.param
    kinds = SETS[name]
    rng = np.random.default_rng(3000 + W + len(kinds))
    counts = ragged_counts(rng, W * H)
    offsets = ref.offsets_ref(counts)
    owners = ref.owners_ref(counts, int(offsets[-1]))
    fields = make_fields(rng, kinds, int(offsets[-1]))
    B = States(W, H, kinds)
    run_compact_arrays(gpu, B, offsets, fields)
    want = B.snapshot()
    R = States(W, H, kinds)
    run_records_ilv(gpu, R, pack(fields, OFFSETS[name], 48, owners=owners, pixel_offset=44), 48, OFFSETS[name], 44)
    same(want, R.snapshot(), "the two yardsticks")
    return W, H, name, kinds, counts, offsets, owners, fields, want


@pytest.mark.parametrize("stride", [44, 48], ids=["tight44", "padded48"])
def test_ragged_counts_equal_both_yardsticks(gpu, ragged, stride):
    W, H, name, kinds, counts, offsets, owners, fields, want = ragged
    assert (counts == 0).mean() > 0.1 and counts.max() == 300
    rec = pack(fields, OFFSETS[name], stride, owners=owners if stride == 48 else None, pixel_offset=44)
    for path in paths_of(name == "five"):
        A = States(W, H, kinds)
        assert_path(gpu, run_ilv(gpu, A, rec, stride, OFFSETS[name], offsets, path=path), path, name == "five", INT32_MAX)
        assert np.array_equal(A.st[0]["n"].cpu().numpy().reshape(-1), counts)
        A = States(W, H, kinds)
        run_ilv(gpu, A, rec, stride, OFFSETS[name], offsets, path=path)
        same(want, A.snapshot(), "path %s" % path)


def test_ragged_counts_match_the_oracle(gpu, oracle):
    W, H = FILMS[0]
    rng = np.random.default_rng(3100)
    counts = ragged_counts(rng, W * H)
    offsets = ref.offsets_ref(counts)
    owners = ref.owners_ref(counts, int(offsets[-1]))
    for kinds, name in ((arrays_tests.TYPES, "four"), (FIVE, "five")):
        samples = arrays_tests.make_samples(rng, int(offsets[-1]), kinds)
        rec = pack(samples, OFFSETS[name], 44)
        for path in paths_of(name == "five"):
            S = arrays_tests.States(W, H, types=kinds)
            layout = gpu.make_record_layout(44, 0, OFFSETS[name])
            sts = [gpu.make_stat_type_record_field(k[1], S.st[i], k[2], k[3], prepass_into=S.pre(i)) for i, k in enumerate(kinds)]
            gpu.compact_interleaved_path(PATHS.index(path))
            try:
                gpu.compact_accumulate_interleaved(W, H, sts, dev(rec), layout, dev(offsets), split_above=INT32_MAX)
            finally:
                gpu.compact_interleaved_path(0)
            arrays_tests.assert_matches_the_oracle(oracle, S, counts, owners, samples)


# ---------------------------------------------------------------- staging edges
# What these cases pin is the RESULT at the edges of the staging rule, under the staged KERNEL: the debug getter names the kernel of
# the launch, not what a wave did, and a staged kernel whose waves never took the LDS path would leave the same bits.  That waves do
# stage here follows from the rule restated on the offsets (tools/time_accumulate_compact_interleaved.py, `staged_wave_share`) and
# from the timings of DESIGN.md 4.1k, not from an assertion in this file.
@pytest.mark.parametrize("stride", [28, 44, 48, 52])
def test_a_span_that_fits_the_window_exactly_and_one_record_more(gpu, stride):
    """The window set to what one record on each of a wave's 64 pixels takes (a multiple of 1024 at every stride here times 16):
    uniform counts fill it to the byte with skew 0; one record more in any wave, or a base 4, 8 or 12 bytes on, does not fit."""
    W, H = 64, 32
    per = 16                                   # records per pixel: 64 * 16 * stride is a multiple of 1024 for every stride
    window = 64 * per * stride
    assert window % 1024 == 0 and window <= 65536
    rng = np.random.default_rng(3200 + stride)
    # 28 bytes: the half-features record (radiance fp32, two RGB and two 1-channel half fields)
    offs, formats = ((0, 12, 18, 24, 26), [F32, F16, F16, F16, F16]) if stride == 28 else (OFFSETS["five"], None)
    try:
        gpu.compact_interleaved_window(window)
        for extra in (0, 1):
            counts = np.full(W * H, per)
            if extra:
                counts[64 * 3 + 17] += 1       # one wave a record too long, between waves that fit
                counts[W * H - 1] += 1
            fields = [np.clip(f, 0, 60000) for f in make_fields(rng, FIVE, int(counts.sum()))]
            for front in (0, 4, 8, 12):
                hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, offs, stride, formats=formats, fusable=True, front=front, back=64)
    finally:
        gpu.compact_interleaved_window(0)


@pytest.mark.parametrize("film", FILMS, ids=lambda f: "%dx%d" % f)
@pytest.mark.parametrize("stride", [28, 44, 48, 52])
def test_short_runs_stage_under_the_default_window(gpu, film, stride):
    """Counts 0 .. 9: every wave's span fits, the last wave of 37 x 29 is partial; one wave holds a run of 700 records (too long for
    any window) between staging neighbours.  Half features in 28 bytes, fp32 elsewhere; the base at every 4-byte phase."""
    W, H = film
    rng = np.random.default_rng(3300 + stride + W)
    counts = rng.integers(0, 10, W * H).astype(np.int64)
    counts[64 * 5 + 31] = 700
    n = int(counts.sum())
    if stride == 28:        # the half-features record: radiance fp32, two RGB half fields, two 1-channel half fields
        offs, formats = (0, 12, 18, 24, 26), [F32, F16, F16, F16, F16]
    else:
        offs, formats = OFFSETS["five"], None
    fields = [np.clip(f, 0, 60000) for f in make_fields(rng, FIVE, n)]
    for front in (0, 4, 8, 12):
        hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, offs, stride, formats=formats, fusable=True, front=front, back=32)


# ---------------------------------------------------------------- run lengths at the walk's batch edges
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_run_lengths_at_the_batch_edges_for_every_kind(gpu, half):
    """0, 1, batch - 1, batch, batch + 1, 2 batch - 1, 2 batch, 2 batch + 1 (and three whole batches with and without a tail) on
    consecutive pixels, all twelve (channels, transform, max_moment) kinds in one call: the 24 bodies of the general fold."""
    W, H = FILMS[0]
    rng = np.random.default_rng(3400)
    edges = [0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH, 2 * BATCH + 1, 3 * BATCH, 3 * BATCH + 1]
    counts = np.resize(np.array(edges), W * H)
    fields = make_fields(rng, KINDS, int(counts.sum()))
    if half:
        fields = [np.clip(f, 0, 60000) for f in fields]
    elem = 2 if half else 4
    offs, at = [], 0
    for k in KINDS:
        offs.append(at)
        at += k[1] * elem
    stride = (at + 3) // 4 * 4
    hold_to_the_compact_entry(gpu, W, H, KINDS, counts, fields, offs, stride, formats=[F16] * len(KINDS) if half else None)


@pytest.mark.parametrize("formats", [None, [F32] + [F16] * 4, [F16] * 5], ids=["fmt0", "fmt1", "fmt2"])
def test_run_lengths_at_the_batch_edges_in_the_fused_fold(gpu, formats):
    W, H = FILMS[1]
    rng = np.random.default_rng(3500)
    edges = [0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH, 2 * BATCH + 1, 3 * BATCH, 3 * BATCH + 1]
    counts = np.resize(np.array(edges), W * H)
    fields = [np.clip(f, 0, 60000) for f in make_fields(rng, FIVE, int(counts.sum()))]
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, OFFSETS["five"], 44, formats=formats, fusable=True)


# ---------------------------------------------------------------- layouts
@pytest.fixture(scope="module")
def small(gpu):
    W, H = FILMS[0]
    rng = np.random.default_rng(3600)
    counts = ragged_counts(rng, W * H)
    return W, H, counts, [np.clip(f, 0, 60000) for f in make_fields(rng, FIVE, int(counts.sum()))]


def test_fields_in_reverse_order_and_padding_between_fields(gpu, small):
    W, H, counts, fields = small
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (32, 20, 8, 4, 0), 44, fusable=True)
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (4, 20, 36, 52, 60), 68, fusable=True)
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (8, 24, 38, 46, 50), 52, formats=[F32, F16, F16, F16, F16], fusable=True)   # halves at odd halfwords
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (2, 10, 16, 22, 24), 28, formats=[F16] * 5, fusable=True)


def test_two_types_read_the_same_field(gpu, small):
    """The radiance field feeds the transform type and a plain RGB type, and a 1-channel type reads its first channel."""
    W, H, counts, fields = small
    shared = [fields[0], fields[0], fields[2], fields[0][:, :1], fields[4]]
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, shared, (0, 0, 12, 0, 24), 28, fusable=True)


def test_a_mixed_format_set_takes_the_general_kernel(gpu, small):
    W, H, counts, fields = small
    formats = [F32, F16, F32, F16, F32]
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (0, 12, 20, 32, 36), 40, formats=formats, fusable=False)
    hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, (0, 8, 20, 32, 36), 40, formats=[F16, F32, F32, F32, F32], fusable=False)


def test_half_fields_widen_exactly(gpu, small):
    """A half depth field holding subnormals, +-65504 and +-0 among ordinary values: the yardstick is handed numpy's exact widening
    as an fp32 arena."""
    W, H, counts, fields = small
    special = np.array([2.0 ** -24, -2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 65504.0, -65504.0, 0.0, -0.0, 2.0 ** -15, 1.0 / 3.0], np.float32)
    depth = fields[3].copy()
    depth[:, 0] = np.resize(special, depth.shape[0])
    fields = fields[:3] + [depth, fields[4]]
    for formats, offs, stride in (([F32, F16, F16, F16, F16], (0, 12, 18, 24, 26), 28), ([F16] * 5, (0, 6, 12, 18, 20), 24)):
        want = hold_to_the_compact_entry(gpu, W, H, FIVE, counts, fields, offs, stride, formats=formats, fusable=True)
        exact = [f.astype(np.float16).astype(np.float32) if fmt == F16 else f for f, fmt in zip(fields, formats)]
        B = States(W, H, FIVE)
        run_compact_arrays(gpu, B, ref.offsets_ref(counts), exact)
        same(want, B.snapshot(), "widened by numpy")


def test_a_garbage_pixel_offset_changes_nothing(gpu, small):
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    rec = pack(fields, OFFSETS["five"], 44)
    for path in PATHS:
        A = States(W, H, FIVE)
        run_ilv(gpu, A, rec, 44, OFFSETS["five"], offsets, path=path)
        first = A.snapshot()
        for garbage in (-4, 3, 44, 1 << 30, -(1 << 31)):
            B = States(W, H, FIVE)
            assert_path(gpu, run_ilv(gpu, B, rec, 44, OFFSETS["five"], offsets, path=path, pixel_offset=garbage), path, True, INT32_MAX)
            same(first, B.snapshot(), "pixel_offset %d" % garbage)


# ---------------------------------------------------------------- split
@pytest.mark.parametrize("name", ["five", "four"])
def test_runs_above_split_above_equal_the_split_records_entry(gpu, name):
    W, H = FILMS[1]
    kinds = SETS[name]
    rng = np.random.default_rng(3700)
    counts = rng.integers(0, 9, W * H).astype(np.int64)
    counts[700], counts[701], counts[710], counts[713], counts[1500] = 8, 9, 64, 65, 300      # 8 is not above 8; three split pixels in one wave
    offsets = ref.offsets_ref(counts)
    owners = ref.owners_ref(counts, int(offsets[-1]))
    fields = make_fields(rng, kinds, int(offsets[-1]))
    split = hold_to_the_compact_entry(gpu, W, H, kinds, counts, fields, OFFSETS[name], 48, fusable=name == "five", split_above=8)
    R = States(W, H, kinds)
    run_records_ilv(gpu, R, pack(fields, OFFSETS[name], 48, owners=owners, pixel_offset=44), 48, OFFSETS[name], 44, split_above=8)
    same(split, R.snapshot(), "statmc_accumulate_records_interleaved_split")
    sequential = hold_to_the_compact_entry(gpu, W, H, kinds, counts, fields, OFFSETS[name], 48, fusable=name == "five")
    R = States(W, H, kinds)
    run_records_arrays(gpu, R, owners, fields)
    same(sequential, R.snapshot(), "statmc_accumulate_records")
    nothing_above = hold_to_the_compact_entry(gpu, W, H, kinds, counts, fields, OFFSETS[name], 48, fusable=name == "five", split_above=300)
    same(sequential, nothing_above, "split_above = the longest run")


# ---------------------------------------------------------------- continued state, epilogue, untouched pixels
def test_the_fold_continues_the_state_and_the_epilogue_is_statmc_prepass(gpu, small):
    api = gpu
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    owners = ref.owners_ref(counts, int(offsets[-1]))
    earlier = make_fields(np.random.default_rng(3800), FIVE, 2 * W * H)
    twice = np.repeat(np.arange(W * H, dtype=np.int32), 2)
    B = States(W, H, FIVE)
    run_records_arrays(api, B, np.concatenate([twice, owners]), [np.concatenate([e, f]) for e, f in zip(earlier, fields)])
    want = B.snapshot()
    rec = pack(fields, OFFSETS["five"], 44)
    for path in PATHS:
        A = States(W, H, FIVE)
        run_records_arrays(api, A, twice, earlier)
        for img in A.pre_images[0]:
            img.fill_(7.0)
        assert_path(api, run_ilv(api, A, rec, 44, OFFSETS["five"], offsets, path=path), path, True, INT32_MAX)
        assert np.array_equal(A.st[0]["n"].cpu().numpy().reshape(-1), counts + 2)
        got = A.snapshot()
        same(want[:-2], got[:-2], "path %s" % path)
        mc, dc = arrays_tests.prepass_of(api, A.st[0], 3)
        touched = (counts > 0).reshape(H, W)
        for have, expect in zip(A.pre_images[0], (mc, dc)):
            g, w = bits(have), bits(expect)
            assert np.array_equal(g[touched], w[touched])
            assert (g[~touched] == np.float32(7.0).view(np.int32)).all()


def test_untouched_pixels_keep_every_bit(gpu, small):
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    rec = pack(fields, OFFSETS["five"], 44)
    untouched = counts == 0
    assert untouched.any()
    for path in PATHS:
        S = FilledStates(W, H, FIVE)          # a random bit pattern in every image: the untouched pixels must keep it
        before = S.snapshot()
        assert_path(gpu, run_ilv(gpu, S, rec, 44, OFFSETS["five"], offsets, path=path, split_above=8), path, True, 8)
        after = S.snapshot()
        for x, y in zip(before, after):       # every image, mean_corr / discriminator included
            assert np.array_equal(x.reshape(W * H, -1)[untouched], y.reshape(W * H, -1)[untouched])
        assert np.array_equal(after[0].reshape(-1) - before[0].reshape(-1), counts)


# ---------------------------------------------------------------- offsets outside the arena
@pytest.mark.parametrize("name", ["five", "four"])
def test_wrong_offsets_are_clamped_before_they_become_addresses(gpu, name):
    """Negative leading offsets, a decreasing pair and trailing offsets beyond n_records: the result is the records entry on the
    clamped runs.  The records lie between guard bands of 0xFF bytes -- NaN in either format --, longer than the largest wrong
    offset: a kernel that clamps late reads memory that exists and fails by its bits."""
    W, H = FILMS[1]
    kinds = SETS[name]
    rng = np.random.default_rng(3900)
    counts = rng.integers(0, 10, W * H).astype(np.int64)
    good = ref.offsets_ref(counts)
    total = int(good[-1])
    fields = make_fields(rng, kinds, total)
    wrong = good.copy()
    wrong[:70] -= 400                      # a wave and more of negative leading offsets
    wrong[200] = wrong[199] - 30
    wrong[-130:] += 500                    # two waves of trailing offsets beyond the arena
    wrong[-1] = total + 100000
    start, end = ref.clamp_runs(wrong, total)
    assert wrong.min() < 0 and wrong.max() > total and (np.diff(wrong) < 0).any() and (start <= end).all()
    pixels, positions = ref.records_of_runs(start, end)
    B = States(W, H, kinds)
    run_records_arrays(gpu, B, pixels, [f[positions] for f in fields])
    want = B.snapshot()
    rec = pack(fields, OFFSETS[name], 44)
    guard = 110000 * 44
    for path in paths_of(name == "five"):
        for split_above in (INT32_MAX, 1000):
            A = States(W, H, kinds)
            got = run_ilv(gpu, A, rec, 44, OFFSETS[name], wrong, path=path, split_above=split_above, front=500 * 44, back=guard)
            assert_path(gpu, got, path, name == "five", split_above)
            same(want, A.snapshot(), "path %s" % path)
    # n_records below the arena's length: the records behind it are guard too
    cut = total - 77
    start, end = ref.clamp_runs(good, cut)
    pixels, positions = ref.records_of_runs(start, end)
    B = States(W, H, kinds)
    run_records_arrays(gpu, B, pixels, [f[positions] for f in fields])
    poisoned = rec.copy()
    poisoned[cut * 44:] = 0xFF
    for path in paths_of(name == "five"):
        A = States(W, H, kinds)
        assert_path(gpu, run_ilv(gpu, A, poisoned, 44, OFFSETS[name], good, n_records=cut, path=path, front=48, back=48), path, name == "five", INT32_MAX)
        same(B.snapshot(), A.snapshot(), "path %s" % path)


# ---------------------------------------------------------------- limits
def test_one_type_and_sixteen_types(gpu):
    W, H = FILMS[0]
    rng = np.random.default_rng(4000)
    counts = ragged_counts(rng, W * H)
    one = [FIVE[0]]
    hold_to_the_compact_entry(gpu, W, H, one, counts, make_fields(rng, one, int(counts.sum())), (4,), 20)
    sixteen = KINDS + KINDS[:4]
    offs, at = [], 0
    for k in sixteen:
        offs.append(at)
        at += 4 * k[1]
    hold_to_the_compact_entry(gpu, W, H, sixteen, counts, make_fields(rng, sixteen, int(counts.sum())), offs, at)


def test_no_records_or_no_types_is_a_no_op(gpu, small):
    import torch
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    S = FilledStates(W, H, FIVE)
    before = S.snapshot()
    for path in PATHS:
        assert run_ilv(gpu, S, pack([f[:0] for f in fields], OFFSETS["five"], 44), 44, OFFSETS["five"], np.zeros(W * H + 1, np.int64), path=path) == 0
        same(before, S.snapshot())
    rec = dev(pack(fields, OFFSETS["five"], 44))
    gpu.compact_accumulate_interleaved(W, H, [], rec, gpu.make_record_layout(44, 0, []), dev(offsets))
    torch.cuda.synchronize()
    assert gpu.last_compact_interleaved_path() == 0
    same(before, S.snapshot())
    lib = gpu.load()
    assert lib.statmc_compact_accumulate_interleaved(W, H, None, 0, None, None, None, 0, 256, None) == 0
    assert lib.statmc_compact_accumulate_interleaved(W, H, None, 5, None, None, None, 0, 256, None) == 0
    assert lib.statmc_compact_accumulate_interleaved(W, H, None, 5, None, None, None, 10, 256, None) == gpu.ERR_INVALID
    same(before, S.snapshot())


def test_identical_calls_give_identical_bits(gpu, small):
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    rec = pack(fields, OFFSETS["five"], 48)
    for path in PATHS:
        shots = []
        for run in range(2):
            S = States(W, H, FIVE)
            assert_path(gpu, run_ilv(gpu, S, rec, 48, OFFSETS["five"], offsets, path=path, split_above=64), path, True, 64)
            shots.append(S.snapshot())
        same(shots[0], shots[1], "path %s" % path)


def test_on_a_side_stream(gpu, small):
    """On a statmc_stream_create side stream while torch's current stream is the null stream; records and offsets are copied in on
    that side stream just before the call.  Equals the null-stream result."""
    import ctypes as C
    import torch
    api, lib = gpu, gpu.load()
    W, H, counts, fields = small
    offsets = ref.offsets_ref(counts)
    rec = pack(fields, OFFSETS["five"], 44)
    assert torch.cuda.current_stream().cuda_stream == 0
    B = States(W, H, FIVE)
    run_ilv(api, B, rec, 44, OFFSETS["five"], offsets, split_above=64)
    want = B.snapshot()
    layout = api.make_record_layout(44, 0, OFFSETS["five"])
    side = C.c_void_p()
    api.check(lib.statmc_stream_create(C.byref(side)))
    try:
        for path in PATHS:
            S = States(W, H, FIVE)
            d_rec = torch.zeros(rec.size, dtype=torch.uint8, device="cuda:0")
            d_off = torch.zeros(offsets.size, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            for dst, src in ((d_rec, rec), (d_off, offsets)):
                api.check(lib.statmc_upload(dst.data_ptr(), src.ctypes.data, src.nbytes, side))
            api.compact_interleaved_path(PATHS.index(path))
            try:
                api.compact_accumulate_interleaved(W, H, field_types(api, S), d_rec, layout, d_off, split_above=64, stream=side)
            finally:
                api.compact_interleaved_path(0)
            api.check(lib.statmc_synchronize(side))
            same(want, S.snapshot(), "path %s" % path)
    finally:
        api.check(lib.statmc_synchronize(side))
        api.check(lib.statmc_stream_destroy(side))


# ---------------------------------------------------------------- the wrappers
def test_filmstats_accumulate_compact_with_records(gpu):
    import torch
    from statmc_amd import film
    api = gpu
    W, H = FILMS[0]
    rng = np.random.default_rng(4100)
    counts = ragged_counts(rng, W * H)
    total = int(counts.sum())
    names = ("radiance", "normal", "albedo")
    host = [arrays_tests.make_samples(rng, total, [arrays_tests.TYPES[0]])[0], rng.random((total, 3)).astype(np.float32),
            rng.random((total, 3)).astype(np.float32)]
    offs, formats = (0, 12, 20), [F32, F16, F16]
    rec = dev(pack(host, offs, 28, formats))
    offsets, _ = api.compact_offsets(dev(counts.astype(np.int32).reshape(H, W)))
    fs = film.FilmStats(W, H, torch.device("cuda:0"), types=names)
    fs.accumulate_compact(offsets=offsets, records=rec, layout=(28, {"radiance": 0, "normal": (12, api.SAMPLES_F16), "albedo": (20, api.SAMPLES_F16)}))
    assert api.last_compact_interleaved_path() & api.COMPACT_ILV_PATH_SPLIT      # the wrapper's default: STATMC_RECORDS_SPLIT_DEFAULT
    st = {t: film.new_state(H, W, 3, torch.device("cuda:0"), transform=film.STAT_TYPES[t]["transform"]) for t in names}
    sts = [api.make_stat_type_record_field(3, st[t], film.STAT_TYPES[t]["transform"], film.STAT_TYPES[t]["max_moment"]) for t in names]
    api.compact_accumulate_interleaved(W, H, sts, rec, api.make_record_layout(28, 0, offs, formats), offsets)
    torch.cuda.synchronize()
    for t in names:
        for k in arrays_tests.FIELDS:
            if st[t].get(k) is not None:
                assert np.array_equal(bits(fs.state[t][k]), bits(st[t][k])), (t, k)
    assert np.array_equal(fs.state["normal"]["n"].cpu().numpy().reshape(-1), counts)
    with pytest.raises(ValueError):
        fs.accumulate_compact(offsets=offsets, records=rec)


def test_estimator_accumulate_compact_interleaved_equals_accumulate_compact(gpu):
    """Estimator::AccumulateCompactInterleaved against Estimator::AccumulateCompact on the de-interleaved arenas
    (tests/cpp/test_compact_accumulate_interleaved.cpp)."""
    from statmc_amd import build
    build.build_tools()
    for w, h in ((61, 37), (96, 64)):
        out = subprocess.run([build.COMPACT_ILV_BIN, str(w), str(h)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "compact accumulate interleaved ok" in out.stdout
