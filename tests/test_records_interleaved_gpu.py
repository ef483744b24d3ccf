"""statmc_accumulate_records_interleaved on the GPU.  The entry is defined by statmc_accumulate_records: it leaves, bit for bit,
what that entry leaves when given every record's pixel and, per stat type, the record-major array of the type's field with half
fields widened to fp32.  So every test here packs numpy fields into a record buffer (api.pack_records), runs the new entry on it
and the old one on the arrays, both from the same seeded random bit pattern in every image (the counts brought into a range a
fold can continue), and compares every state image, mean_corr and discriminator bitwise -- through the general kernel, through
the fused kernel where the type set is eligible for it, and with the kernel left to the library."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILMS = [(37, 29), (64, 32)]
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
# (name, channels, transform, max_moment, pre-pass epilogue)
FOUR = [("radiance", 3, 1, 3, True), ("normal", 3, 0, 1, False), ("depth", 1, 0, 1, False), ("extra", 1, 1, 2, False)]   # tests/test_records_gpu.py's: general only
FIVE = [("radiance", 3, 1, 3, True), ("albedo", 3, 0, 1, False), ("normal", 3, 0, 1, False), ("depth", 1, 0, 1, False),
        ("id", 1, 0, 1, False)]                                                                                       # the shipped 11-channel set: fused
SETS = {"four": FOUR, "five": FIVE}
F32, F16 = 0, 1
AUTO, GENERAL, FUSED = 0, 1, 2


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


class States:
    """One set of state images per stat type of `kinds`, plus mean_corr / discriminator for the types with the epilogue; every
    image starts from a random bit pattern that depends on `seed` alone (fill=False: zeros)."""

    def __init__(self, W, H, kinds, seed=77, fill=True):
        import torch
        from statmc_amd import film
        self.W, self.H, self.kinds = W, H, kinds
        self.st = [film.new_state(H, W, c, torch.device("cuda:0"), transform=bool(t)) for _, c, t, _, _ in kinds]
        self.pre_images = [(torch.zeros(H, W, c, device="cuda:0"), torch.zeros(H, W, c, device="cuda:0")) if pre else None
                           for _, c, _, _, pre in kinds]
        if fill:
            rng = np.random.default_rng(seed)
            for img in self.images():
                raw = rng.integers(-2 ** 31, 2 ** 31, size=tuple(img.shape), dtype=np.int64).astype(np.int32)
                img.copy_(dev(raw).view(img.dtype))
            for st in self.st:
                st["n"].remainder_(1000).abs_()

    def images(self):
        out = []
        for st in self.st:
            out += [st[k] for k in FIELDS if st.get(k) is not None]
        for pre in self.pre_images:
            if pre is not None:
                out += list(pre)
        return out

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        return [bits(img).copy() for img in self.images()]


def same(a, b, what=""):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s: image %d differs in %d elements" % (what, k, int((x != y).sum()))


def make_fields(rng, kinds, n):
    """Per type [n, C] fp32: log-normal, a fifth exact zeros, one x 1000 value (tests/test_records_gpu.py's samples)."""
    out = []
    for _, c, _, _, _ in kinds:
        s = np.exp(rng.normal(0.0, 1.0, (n, c))).astype(np.float32)
        s[rng.random((n, c)) < 0.2] = 0.0
        if n:
            s[int(rng.integers(0, n))] *= np.float32(1000.0)
        out.append(s)
    return out


def records_of_counts(rng, counts, dead=0.0):
    npx = counts.size
    px = np.repeat(np.arange(npx, dtype=np.int32), counts)
    n_dead = int(round(dead * px.size))
    marks = np.where(np.arange(n_dead) % 2 == 0, -1, npx + 7).astype(np.int32)
    px = np.concatenate([px, marks])
    return px[rng.permutation(px.size)]


def ragged_counts(rng, npx):
    """0 .. 9 records per pixel, about a fifth of the pixels at 0, one pixel at 300"""
    counts = rng.integers(1, 10, npx).astype(np.int64)
    counts[rng.random(npx) < 0.2] = 0
    counts[int(rng.integers(0, npx))] = 300
    return counts


def widened(fields, formats):
    """what the definition hands the yardstick: half fields rounded to half (as pack_records rounds them) and widened to fp32"""
    if formats is None:
        return fields
    return [f.astype(np.float16).astype(np.float32) if fmt == F16 else f for f, fmt in zip(fields, formats)]


def run_arrays(api, S, pixels, fields, lo=0, hi=None):
    """the yardstick: statmc_accumulate_records on one array per type"""
    import torch
    hi = len(pixels) if hi is None else hi
    d_px = dev(pixels[lo:hi])
    d_s = [dev(f[lo:hi]) for f in fields]
    sts = [api.make_stat_type_records(d_s[i], k[1], S.st[i], k[2], k[3], prepass_into=S.pre_images[i]) for i, k in enumerate(S.kinds)]
    api.accumulate_records(S.W, S.H, sts, d_px)
    torch.cuda.synchronize()


def run_interleaved(api, S, rec, layout, path=AUTO, lo=0, hi=None, shift=0):
    """records [lo, hi) of the packed buffer `rec` (numpy uint8); shift: the records start that many bytes into their tensor"""
    import torch
    stride = layout.stride
    hi = rec.size // stride if hi is None else hi
    buf = np.concatenate([np.zeros(shift, np.uint8), rec[lo * stride:hi * stride]])
    d_rec = dev(buf)[shift:]
    assert d_rec.data_ptr() % 16 == shift % 16
    sts = [api.make_stat_type_record_field(k[1], S.st[i], k[2], k[3], prepass_into=S.pre_images[i]) for i, k in enumerate(S.kinds)]
    api.accumulate_records_interleaved_path(path)
    try:
        api.accumulate_records_interleaved(S.W, S.H, sts, d_rec, layout, n_records=hi - lo)
        torch.cuda.synchronize()
    finally:
        api.accumulate_records_interleaved_path(AUTO)
    return api.last_accumulate_records_interleaved_path()


def check_case(api, W, H, kinds, pixels, fields, formats=None, fusable=False, shift=0, **pack):
    """The new entry on the packed records against the old one on the arrays, through every path."""
    ref = States(W, H, kinds)
    run_arrays(api, ref, pixels, widened(fields, formats))
    want = ref.snapshot()
    rec, layout = api.pack_records(pixels, fields, formats=formats, fill=0xEE, **pack)
    for path in (AUTO, GENERAL, FUSED):
        S = States(W, H, kinds)
        took = run_interleaved(api, S, rec, layout, path, shift=shift)
        if len(pixels):
            assert took == (FUSED if fusable and path != GENERAL else GENERAL), (path, took)
        same(want, S.snapshot(), "path %d" % path)
    return want


def fusable_formats(kinds, formats):
    """the fused kernel's format classes for the FIVE set: all fp32, or every feature half (the radiance field either)"""
    if kinds is not FIVE:
        return False
    return formats is None or all(f == F16 for f in formats[1:]) or all(f == F32 for f in formats)


@pytest.fixture(scope="module", params=[(f, s) for f in FILMS for s in SETS], ids=lambda p: "%dx%d-%s" % (p[0][0], p[0][1], p[1]))
def ragged(request, gpu):
    """One ragged record set per film and type set: counts 0 .. 9 with one pixel at 300, a fifth of the pixels empty, a tenth of
    the records dead (-1 and npx + 7), shuffled."""
    (W, H), set_name = request.param
    kinds = SETS[set_name]
    rng = np.random.default_rng(2000 + W + len(kinds))
    counts = ragged_counts(rng, W * H)
    pixels = records_of_counts(rng, counts, dead=0.1)
    fields = make_fields(rng, kinds, pixels.size)
    return W, H, kinds, counts, pixels, fields


def half_features(kinds):
    return [F32] + [F16] * (len(kinds) - 1)


def test_ragged_counts_tight_records(gpu, ragged):
    W, H, kinds, counts, pixels, fields = ragged
    assert (counts == 0).mean() > 0.1 and counts.max() == 300
    assert (pixels == -1).any() and (pixels == W * H + 7).any()
    want = check_case(gpu, W, H, kinds, pixels, fields, fusable=kinds is FIVE)
    # the counts moved by what was fed: nothing lost, nothing folded twice, no dead record folded
    start = States(W, H, kinds).snapshot()
    assert np.array_equal(want[0].reshape(-1) - start[0].reshape(-1), counts)
    if kinds is FIVE:
        rec, layout = gpu.pack_records(pixels, fields)
        assert layout.stride == 48


@pytest.mark.parametrize("layout_case", ["pad4", "stride64", "half", "reversed", "pixel_mid", "half_odd2", "all_half", "rad_half_only"])
def test_layouts(gpu, ragged, layout_case):
    W, H, kinds, counts, pixels, fields = ragged
    sizes = [4 * k[1] for k in kinds]
    tight = 4 + sum(sizes)
    formats, pack = None, {}
    if layout_case == "pad4":                      # 52 for the 11-channel set: padding behind the last field
        pack = dict(stride=tight + 4)
    elif layout_case == "stride64":
        pack = dict(stride=64)
    elif layout_case == "half":                    # radiance fp32, the features half: 28 bytes of samples behind the pixel index
        formats = half_features(kinds)
    elif layout_case == "reversed":                # the fields in reversed order behind the pixel
        offs, at = [], 4
        for sz in reversed(sizes):
            offs.append(at)
            at += sz
        pack = dict(offsets=list(reversed(offs)))
    elif layout_case == "pixel_mid":               # the pixel index between the first field and the rest
        offs, at = [0], sizes[0] + 4
        for sz in sizes[1:]:
            offs.append(at)
            at += sz
        pack = dict(offsets=offs, pixel_offset=sizes[0])
    elif layout_case == "half_odd2":               # every half field at an offset that is a multiple of 2 but not of 4
        formats = half_features(kinds)
        offs, at = [4], 16
        for k in kinds[1:]:
            at = (at + 3) // 4 * 4 + 2
            offs.append(at)
            at += 2 * k[1]
        assert all(o % 4 == 2 for o in offs[1:])
        pack = dict(offsets=offs)
    elif layout_case == "all_half":
        formats = [F16] * len(kinds)
    elif layout_case == "rad_half_only":           # a mix the fused kernel does not take
        formats = [F16] + [F32] * (len(kinds) - 1)
    if formats is not None and formats[0] == F16:  # radiance a clamping renderer could hold in half
        fields = [np.minimum(fields[0], np.float32(60000.0))] + fields[1:]
    check_case(gpu, W, H, kinds, pixels, fields, formats=formats, fusable=fusable_formats(kinds, formats), **pack)
    if kinds is FIVE and layout_case in ("half", "all_half"):   # 4 + 12 + 16 = 32 bytes; 4 + 22 = 26, padded to 28
        assert gpu.pack_records(pixels, fields, formats=formats)[1].stride == (32 if layout_case == "half" else 28)


def test_records_at_a_4_byte_aligned_address(gpu, ragged):
    W, H, kinds, counts, pixels, fields = ragged
    for shift in (4, 12):
        check_case(gpu, W, H, kinds, pixels, fields, fusable=kinds is FIVE, shift=shift)


def test_every_kind_at_the_walks_edges_in_the_general_fold(gpu):
    """All 24 bodies of the general fold's type dispatch -- twelve (channels, transform, max_moment) kinds, every field fp32 and
    every field half -- on runs at every edge of the walk (tests/test_records_gpu.py's lengths): bit-equal to
    statmc_accumulate_records on the de-interleaved arrays that hold the widened values."""
    W, H = 16, 8
    from test_records_gpu import KINDS as kinds
    rng = np.random.default_rng(43)
    counts = np.resize(np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17]), W * H)
    pixels = records_of_counts(rng, counts, dead=0.05)
    fields = [np.minimum(f, np.float32(60000.0)) for f in make_fields(rng, kinds, pixels.size)]      # finite in half
    for formats in (None, [F16] * len(kinds)):
        ref = States(W, H, kinds)
        run_arrays(gpu, ref, pixels, widened(fields, formats))
        rec, layout = gpu.pack_records(pixels, fields, formats=formats, fill=0xEE)
        S = States(W, H, kinds)
        assert run_interleaved(gpu, S, rec, layout, GENERAL) == GENERAL
        same(ref.snapshot(), S.snapshot(), "fp32" if formats is None else "half")


@pytest.mark.parametrize("set_name", list(SETS))
def test_run_lengths_at_the_batch_edges(gpu, set_name):
    """Runs of 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13 records on consecutive pixels: shorter than a batch of four, whole batches, an odd
    and an even number of them, each with and without a tail."""
    W, H = 37, 29
    kinds = SETS[set_name]
    rng = np.random.default_rng(31)
    lengths = np.array([1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13])
    counts = np.resize(lengths, W * H)
    pixels = records_of_counts(rng, counts)
    fields = make_fields(rng, kinds, pixels.size)
    check_case(gpu, W, H, kinds, pixels, fields, fusable=kinds is FIVE)
    check_case(gpu, W, H, kinds, pixels, fields, formats=half_features(kinds), fusable=kinds is FIVE)


def test_two_types_read_the_same_field(gpu):
    """The radiance field feeds the transform type and a plain RGB type, and a 1-channel type reads its first channel: three
    overlapping fields, a type set the fused kernel takes (K = 1, M = 1)."""
    W, H = 37, 29
    kinds = [("radiance", 3, 1, 3, True), ("plain", 3, 0, 1, False), ("red", 1, 0, 1, False)]
    rng = np.random.default_rng(41)
    pixels = records_of_counts(rng, ragged_counts(rng, W * H), dead=0.1)
    rad = make_fields(rng, kinds[:1], pixels.size)[0]
    fields = [rad, rad, rad[:, :1].copy()]
    check_case(gpu, W, H, kinds, pixels, fields, fusable=True, offsets=[4, 4, 4])
    # ... and two radiance types on one field: general
    kinds2 = [("radiance", 3, 1, 3, True), ("again", 3, 1, 3, False)]
    check_case(gpu, W, H, kinds2, pixels, [rad, rad], fusable=False, offsets=[8, 8], pixel_offset=4, stride=24)


@pytest.mark.parametrize("set_name", list(SETS))
def test_half_fields_widen_exactly(gpu, set_name):
    """A half depth field holding subnormals, +-65504 and +-0 (and ordinary values): the yardstick gets numpy's exact widening."""
    W, H = 37, 29
    kinds = SETS[set_name]
    rng = np.random.default_rng(51)
    pixels = records_of_counts(rng, ragged_counts(rng, W * H), dead=0.1)
    fields = make_fields(rng, kinds, pixels.size)
    special = np.array([0x0001, 0x8001, 0x03ff, 0x83ff, 0x0200, 0x7bff, 0xfbff, 0x0000, 0x8000, 0x0400, 0x3c00, 0xbc00], np.uint16).view(np.float16)
    assert special[5] == 65504.0 and special[6] == -65504.0 and np.signbit(special[8]) and special[8] == 0
    assert 0 < float(special[0]) < 6.2e-5 and float(special[2]) < 6.2e-5                          # subnormals
    depth = np.resize(special, pixels.size)[rng.permutation(pixels.size)].astype(np.float32).reshape(-1, 1)
    fields[3 if kinds is FIVE else 2] = depth
    check_case(gpu, W, H, kinds, pixels, fields, formats=half_features(kinds), fusable=kinds is FIVE)
    # ... and with every half field in the upper half of a dword (offsets 2 mod 4)
    check_case(gpu, W, H, kinds, pixels, fields, formats=half_features(kinds), fusable=kinds is FIVE,
               offsets=[4] + [18 + 8 * i for i in range(len(kinds) - 1)])


def test_one_type_and_sixteen_types(gpu):
    W, H = 37, 29
    rng = np.random.default_rng(61)
    pixels = records_of_counts(rng, ragged_counts(rng, W * H), dead=0.1)
    one = FOUR[:1]
    check_case(gpu, W, H, one, pixels, make_fields(rng, one, pixels.size), fusable=False)
    # sixteen types over a 44-byte record: every kind of the two sets, several types per field
    base = FIVE + [FOUR[3]]
    sixteen = [(base[i % 6][0] + str(i),) + tuple(base[i % 6][1:4]) + (base[i % 6][4] and i < 6,) for i in range(16)]
    fields6 = make_fields(rng, base, pixels.size)
    fields6[5] = fields6[3]                       # "extra" reads the depth field
    fields = [fields6[i % 6] for i in range(16)]
    offs6 = [4, 16, 28, 40, 44, 40]
    formats6 = [F32, F32, F16, F32, F16, F32]
    fields = [f.astype(np.float16).astype(np.float32) if formats6[i % 6] == F16 else f for i, f in enumerate(fields)]   # overlapping writers agree
    check_case(gpu, W, H, sixteen, pixels, fields, formats=[formats6[i % 6] for i in range(16)], fusable=False,
               offsets=[offs6[i % 6] for i in range(16)], stride=48)


def test_no_records_or_no_types_is_a_no_op(gpu):
    import torch
    api = gpu
    W, H = 37, 29
    S = States(W, H, FIVE, seed=8)
    before = S.snapshot()
    rec, layout = api.pack_records(np.zeros(0, np.int32), make_fields(np.random.default_rng(9), FIVE, 0))
    assert run_interleaved(api, S, rec, layout) == 0                       # zero records: nothing planned, nothing launched
    rec, layout = api.pack_records(np.arange(10, dtype=np.int32), [])
    api.accumulate_records_interleaved(W, H, [], dev(rec), layout)         # zero types
    api.accumulate_records_interleaved(W, H, [], dev(rec), layout, n_records=0)
    torch.cuda.synchronize()
    same(before, S.snapshot())
    # only dead records: the grouping and the fold run, nothing changes anywhere
    dead = np.where(np.arange(50) % 2 == 0, -1, W * H + 7).astype(np.int32)
    rec, layout = api.pack_records(dead, make_fields(np.random.default_rng(10), FIVE, dead.size))
    for path in (GENERAL, FUSED):
        run_interleaved(api, S, rec, layout, path)
        same(before, S.snapshot())


def test_untouched_pixels_keep_every_bit(gpu, ragged):
    W, H, kinds, counts, pixels, fields = ragged
    rec, layout = gpu.pack_records(pixels, fields)
    untouched = counts == 0
    assert untouched.any()
    for path in (GENERAL, FUSED):
        S = States(W, H, kinds, seed=5)
        before = S.snapshot()
        run_interleaved(gpu, S, rec, layout, path)
        after = S.snapshot()
        for x, y in zip(before, after):
            xs, ys = x.reshape(W * H, -1), y.reshape(W * H, -1)
            assert np.array_equal(xs[untouched], ys[untouched])
        assert np.array_equal(after[0].reshape(-1) - before[0].reshape(-1), counts)      # ... and the others were folded


def test_split_calls_and_repeated_calls(gpu, ragged):
    """A call over [0, n) equals calls over [0, m) then [m, n); the same call twice from the same start gives the same bits."""
    W, H, kinds, counts, pixels, fields = ragged
    formats = half_features(kinds)
    ref = States(W, H, kinds)
    run_arrays(gpu, ref, pixels, widened(fields, formats))
    want = ref.snapshot()
    rec, layout = gpu.pack_records(pixels, fields, formats=formats)
    m = len(pixels) // 3
    for path in (GENERAL, FUSED):
        S = States(W, H, kinds)
        run_interleaved(gpu, S, rec, layout, path, 0, m)
        run_interleaved(gpu, S, rec, layout, path, m, None)
        same(want, S.snapshot(), "split, path %d" % path)
        runs = []
        for again in range(2):
            S = States(W, H, kinds)
            run_interleaved(gpu, S, rec, layout, path)
            runs.append(S.snapshot())
        same(runs[0], runs[1], "twice, path %d" % path)
        same(want, runs[0])


def test_the_shipped_set_takes_the_fused_kernel(gpu, ragged):
    """What the library reports about its own choice (statmc_debug_last_accumulate_records_interleaved_path), left to itself."""
    W, H, kinds, counts, pixels, fields = ragged
    for formats in (None, half_features(kinds), [F16] * len(kinds)):
        f = fields if formats is None or formats[0] == F32 else [np.minimum(fields[0], np.float32(60000.0))] + fields[1:]
        rec, layout = gpu.pack_records(pixels, f, formats=formats)
        S = States(W, H, kinds, fill=False)
        assert run_interleaved(gpu, S, rec, layout, AUTO) == (FUSED if kinds is FIVE else GENERAL)
        assert run_interleaved(gpu, S, rec, layout, GENERAL) == GENERAL


def test_phases_apply_to_the_interleaved_entry(gpu, ragged):
    """statmc_debug_accumulate_records_phases: the grouping alone changes no image; the fold alone, over the index it left, completes
    the call."""
    W, H, kinds, counts, pixels, fields = ragged
    lib = gpu.load()
    rec, layout = gpu.pack_records(pixels, fields)
    whole = States(W, H, kinds)
    run_interleaved(gpu, whole, rec, layout)
    S = States(W, H, kinds)
    before = S.snapshot()
    try:
        gpu.check(lib.statmc_debug_accumulate_records_phases(1))
        run_interleaved(gpu, S, rec, layout)
        same(before, S.snapshot())
        gpu.check(lib.statmc_debug_accumulate_records_phases(2))
        run_interleaved(gpu, S, rec, layout)
    finally:
        gpu.check(lib.statmc_debug_accumulate_records_phases(3))
    same(whole.snapshot(), S.snapshot())


def test_estimator_accumulate_records_interleaved_equals_accumulate_records(gpu):
    """C++ host: an Estimator fed through AccumulateRecordsInterleaved holds the bits of one fed the de-interleaved arrays through
    AccumulateRecords, and denoises to the same film-f (tests/cpp/test_accumulate_records_interleaved.cpp)."""
    from statmc_amd import build
    build.build_tools()
    for w, h in ((61, 37), (96, 64)):
        out = subprocess.run([build.REC_ILV_BIN, str(w), str(h)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "accumulate records interleaved ok" in out.stdout
