"""statmc_gather_states / statmc_combine_records on the GPU: the states of listed pixels lifted out of a film as records, and
unordered (pixel, state) records merged into a film -- per pixel in ascending record index, the bits of statmc_combine_statistics /
statmc_combine_many on the same parts in that order, whatever the order of the records of different pixels, and on every run.
All twelve kinds of stat type, the pre-pass epilogue on c3t1m3.  Every comparison is on bits (int32 views of every image)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILMS = [(37, 29), (64, 32)]     # the FILMS of tests/test_records_gpu.py: odd width and a ragged last group / one aligned film
# (name, channels, transform, max_moment, pre-pass epilogue): every (channels, transform, max_moment) a stat type can have
KINDS = [("c%dt%dm%d" % (c, t, m), c, t, m, (c, t, m) == (3, 1, 3)) for c in (3, 1) for t in (1, 0) for m in (3, 2, 1)]
RADIANCE = 0                     # KINDS[0] = c3t1m3
FIELDS = ("n", "mean", "m2", "m3", "film_mean", "film_m2")
INT32_MAX = 2 ** 31 - 1
film_ids = lambda f: "%dx%d" % f


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.int32) if a.dtype == np.float32 else a


def dwords(kind):
    _, c, t, m, _ = kind
    return 1 + c * (m + (2 if t else 0))


class Film:
    """One set of state images per kind, plus the c3t1m3 kind's mean_corr / discriminator."""

    def __init__(self, W, H, fill=None):
        import torch
        from statmc_amd import film
        self.W, self.H = W, H
        self.st = [film.new_state(H, W, c, torch.device("cuda:0"), transform=bool(t)) for _, c, t, _, _ in KINDS]
        self.mc = torch.zeros(H, W, 3, device="cuda:0")
        self.dc = torch.zeros(H, W, 3, device="cuda:0")
        if fill is not None:       # a seeded random bit pattern in every image
            for img in self.images():
                raw = fill.integers(-2 ** 31, 2 ** 31, size=tuple(img.shape), dtype=np.int64).astype(np.int32)
                img.copy_(dev(raw).view(img.dtype))

    def images(self):
        out = []
        for st in self.st:
            out += [st[k] for k in FIELDS if st.get(k) is not None]
        return out + [self.mc, self.dc]

    def snapshot(self):
        import torch
        torch.cuda.synchronize()
        return [bits(img).copy() for img in self.images()]

    def copy(self):
        other = Film(self.W, self.H)
        for a, b in zip(other.images(), self.images()):
            a.copy_(b)
        return other

    def copy_pixels_from(self, other, pixels):
        """every image of `other` at the listed pixels into this film"""
        idx = dev(np.asarray(pixels, np.int64))
        for a, b in zip(self.images(), other.images()):
            c = a.shape[2] if a.dim() == 3 else 1
            a.view(-1, c)[idx] = b.view(-1, c)[idx]

    def pre(self, i):
        return (self.mc, self.dc) if KINDS[i][4] else None

    def types(self, api, prepass=True):
        return [api.make_stat_type_record_field(k[1], self.st[i], k[2], k[3], prepass_into=self.pre(i) if prepass else None)
                for i, k in enumerate(KINDS)]

    def accumulate(self, api, rng, counts):
        """counts[p] samples into pixel p of every kind, through statmc_accumulate_records (the epilogue on c3t1m3)"""
        import torch
        px = np.repeat(np.arange(self.W * self.H, dtype=np.int32), counts)
        px = px[rng.permutation(px.size)]
        smp = make_samples(rng, px.size)
        d_px, d_s = dev(px), [dev(s) for s in smp]
        sts = [api.make_stat_type_records(d_s[i], k[1], self.st[i], k[2], k[3], prepass_into=self.pre(i)) for i, k in enumerate(KINDS)]
        api.accumulate_records(self.W, self.H, sts, d_px)
        torch.cuda.synchronize()
        return self

    def with_current_prepass(self, api):
        """mean_corr / discriminator as the dense entries' epilogue leaves them, on every pixel -- the accumulation's epilogue wrote
        only the pixels that got samples --: a combine with a film of no samples keeps every state bit and writes the pre-pass."""
        self.combine_dense(api, Film(self.W, self.H))
        return self

    def gather(self, api, pixels, stream=None):
        return api.gather_states(self.W, self.H, self.types(api, prepass=False), pixels, stream=stream)

    def combine(self, api, pixels, states, split_above=None, stream=None):
        import torch
        api.combine_records(self.W, self.H, self.types(api), pixels, states, split_above=split_above, stream=stream)
        if stream is None:
            torch.cuda.synchronize()

    def combine_dense(self, api, others):
        """statmc_combine_statistics (one part) or statmc_combine_many (a list), the epilogue on c3t1m3"""
        import torch
        if isinstance(others, Film):
            entries = [api.make_combine_entry(self.st[i], others.st[i], k[1], k[3], prepass_into=self.pre(i)) for i, k in enumerate(KINDS)]
            api.combine_statistics(self.W, self.H, entries)
        else:
            entries = [api.make_combine_many_entry(self.st[i], [o.st[i] for o in others], k[1], k[3], prepass_into=self.pre(i))
                       for i, k in enumerate(KINDS)]
            api.combine_many(self.W, self.H, entries)
        torch.cuda.synchronize()


def same(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s image %d differs in %d elements" % (what, k, int((x != y).sum()))


def make_samples(rng, n):
    """Per kind [n, C] fp32: log-normal, a fifth exact zeros, one x 1000 value (the sample shapes of tests/test_records_gpu.py)."""
    out = []
    for _, c, _, _, _ in KINDS:
        s = np.exp(rng.normal(0.0, 1.0, (n, c))).astype(np.float32)
        s[rng.random((n, c)) < 0.2] = 0.0
        if n:
            s[int(rng.integers(0, n))] *= np.float32(1000.0)
        out.append(s)
    return out


def with_dead(rng, pixels, npx, share=0.05):
    """`pixels` with a share of dead marks mixed in, shuffled"""
    n_dead = max(2, int(round(share * len(pixels))))
    marks = np.array([-1, npx, npx + 7, -2 ** 31, INT32_MAX], np.int64)[np.arange(n_dead) % 5]
    px = np.concatenate([np.asarray(pixels, np.int64), marks]).astype(np.int32)
    return px[rng.permutation(px.size)]


def expected_records(snapshot_of_kind, kind, pixels, npx):
    """The restatement of the record layout: dword 0 the count, then per channel mean, m2, m3, film_mean, film_m2 as far as the
    kind has them; a dead pixel value: all zeros.  snapshot_of_kind: {field: int32 bits}."""
    _, c, t, m, _ = kind
    planes = ["mean"] + (["m2"] if m >= 2 else []) + (["m3"] if m >= 3 else []) + (["film_mean", "film_m2"] if t else [])
    pixels = np.asarray(pixels, np.int64)
    live = (pixels >= 0) & (pixels < npx)
    p = np.where(live, pixels, 0)
    cols = [snapshot_of_kind["n"].reshape(-1)[p]]
    for ch in range(c):
        for f in planes:
            cols.append(snapshot_of_kind[f].reshape(-1, c)[p, ch])
    rec = np.stack(cols, axis=1).astype(np.int32)
    rec[~live] = 0
    assert rec.shape[1] == dwords(kind)
    return rec


def kind_bits(film, i):
    import torch
    torch.cuda.synchronize()
    return {f: bits(film.st[i][f]) for f in FIELDS if film.st[i].get(f) is not None}


# ---------------------------------------------------------------- 1. the gather
@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_gather_lifts_the_listed_states(gpu, film):
    """The records equal the images at the listed pixels (every image a random bit pattern: NaNs, infinities and negative counts
    travel as bits), dead values give the cleared state, duplicates work, and a guard region in front of and behind every
    states[t] -- which starts at an odd dword -- keeps its fill."""
    import torch
    W, H = film
    npx = W * H
    rng = np.random.default_rng(100 + W)
    A = Film(W, H, fill=rng)
    before = A.snapshot()
    pixels = with_dead(rng, rng.integers(0, npx, 700), npx, share=0.1)          # 700 draws from ~1000 / 2000 pixels: duplicates
    pixels[:3] = [0, npx - 1, npx - 1]
    assert np.unique(pixels).size < pixels.size and (pixels == -1).any() and (pixels == npx).any() and (pixels == INT32_MAX).any()
    n, guard, fill = pixels.size, 64, 0x5A5A5A5A
    raw = [torch.full((1 + n * dwords(k) + guard,), fill, dtype=torch.int32, device="cuda:0") for k in KINDS]
    out = [r[1:1 + n * dwords(k)].view(n, dwords(k)) for r, k in zip(raw, KINDS)]
    got = api_gather(gpu, A, dev(pixels), out)
    torch.cuda.synchronize()
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    for i, k in enumerate(KINDS):
        r = raw[i].cpu().numpy()
        assert r[0] == fill and np.all(r[1 + n * dwords(k):] == fill), k[0]
        want = expected_records(kind_bits(A, i), k, pixels, npx)
        assert np.array_equal(r[1:1 + n * dwords(k)].reshape(n, -1), want), k[0]
    same(A.snapshot(), before, "the gather wrote to")
    fresh = A.gather(gpu, dev(pixels))                                          # tensors of the wrapper's own
    torch.cuda.synchronize()
    for g, o in zip(fresh, out):
        assert g.shape == o.shape and torch.equal(g, o)


def api_gather(api, film, pixels, out):
    return api.gather_states(film.W, film.H, film.types(api, prepass=False), pixels, out=out)


# ---------------------------------------------------------------- 2. sparse equals dense
@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_sparse_combine_equals_the_whole_film_combine(gpu, film):
    """Film A: samples everywhere.  Film B: samples on a random third of the pixels.  gather_states(B) at B's touched pixels --
    shuffled, 5 % dead marks -- then combine_records(A) equals statmc_combine_statistics(A, B) in every image, epilogue included."""
    W, H = film
    npx = W * H
    rng = np.random.default_rng(200 + W)
    A = Film(W, H).accumulate(gpu, rng, rng.integers(1, 5, npx))
    touched = rng.random(npx) < 1 / 3
    B = Film(W, H).accumulate(gpu, rng, np.where(touched, rng.integers(1, 5, npx), 0))
    dense = A.copy()
    dense.combine_dense(gpu, B)
    pixels = dev(with_dead(rng, np.flatnonzero(touched), npx))
    A.combine(gpu, pixels, B.gather(gpu, pixels))
    assert int(A.st[RADIANCE]["n"].sum()) == int(dense.st[RADIANCE]["n"].sum()) > 0
    same(A.snapshot(), dense.snapshot())


# ---------------------------------------------------------------- 3. K parts
def records_of_parts(api, rng, parts, listed, npx, order):
    """One record per (part k, pixel listed[k]); per pixel part k before part k + 1 (order = +1) or behind it (-1), the records of
    different pixels interleaved at random, dead marks in between.  Returns (pixels, states) on the device."""
    import torch
    px = np.concatenate([np.asarray(l, np.int64) for l in listed])
    part = np.concatenate([np.full(len(l), k, np.int64) for k, l in enumerate(listed)])
    n_dead = max(2, px.size // 20)
    px = np.concatenate([px, np.array([-1, npx + 7], np.int64)[np.arange(n_dead) % 2]])
    part = np.concatenate([part, np.zeros(n_dead, np.int64)])
    perm = rng.permutation(px.size)
    px, part = px[perm], part[perm]
    # the positions a pixel got, in ascending order, take its parts in ascending (descending) order
    pos = np.argsort(px, kind="stable")
    inner = np.lexsort((order * part[pos], px[pos]))
    part[pos] = part[pos][inner]
    d_px = dev(px.astype(np.int32))
    per_part = [p.gather(api, d_px) for p in parts]                 # [K][kind] -> [n, D]
    pick = dev(part)
    rows = torch.arange(px.size, device="cuda:0")
    states = [torch.stack([per_part[k][i] for k in range(len(parts))])[pick, rows].contiguous() for i in range(len(KINDS))]
    return d_px, states


@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_k_parts_equal_combine_many(gpu, film, K):
    """Records gathered from K films, part k before part k + 1 for every pixel, equal statmc_combine_many -- the left fold --
    whatever the interleaving of different pixels; with the order inside the pixels reversed the last bits change."""
    W, H = film
    npx = W * H
    rng = np.random.default_rng(300 + W + K)
    F = Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx)).with_current_prepass(gpu)      # some pixels start from n = 0
    parts, listed, live = [], [], np.zeros(npx, np.int64)
    for k in range(K):
        touched = rng.random(npx) < 0.7
        parts.append(Film(W, H).accumulate(gpu, rng, np.where(touched, rng.integers(1, 4, npx), 0)))
        listed.append(np.flatnonzero(touched | (rng.random(npx) < 0.1)))       # ... and some records that carry nothing (n = 0)
        live += touched
    dense = F.copy()
    dense.combine_dense(gpu, parts)
    want = dense.snapshot()
    for trial in range(2):                                                     # two interleavings of the records of different pixels
        G = F.copy()
        G.combine(gpu, *records_of_parts(gpu, rng, parts, listed, npx, +1))
        same(G.snapshot(), want, "interleaving %d:" % trial)
    if K == 5:
        R = F.copy()
        R.combine(gpu, *records_of_parts(gpu, rng, parts, listed, npx, -1))
        assert np.array_equal(bits(R.st[RADIANCE]["n"]), bits(dense.st[RADIANCE]["n"]))
        many = live >= 3
        differs = (bits(R.st[RADIANCE]["m3"]) != bits(dense.st[RADIANCE]["m3"])).reshape(npx, 3).any(axis=1)
        print("reversed order: %d of %d pixels with three or more live parts differ in m3" % (int(differs[many].sum()), int(many.sum())))
        assert many.sum() > npx // 2 and differs[many].sum() * 2 >= many.sum()


# ---------------------------------------------------------------- 4. untouched pixels, two calls, two runs
@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_untouched_pixels_two_calls_and_two_runs(gpu, film):
    """Every image pre-filled with random bit patterns; the touched pixels get sane states.  [0, n) equals [0, m) then [m, n); two
    runs give the same bits; pixels without a record, or whose records all have n <= 0 (0 and -3, their fields garbage), keep
    every bit of every image, mean_corr / discriminator included."""
    import torch
    W, H = film
    npx = W * H
    rng = np.random.default_rng(400 + W)
    touched = np.flatnonzero(rng.random(npx) < 0.4)
    barren = np.setdiff1d(np.arange(npx), touched)[::3]                        # records, but none with a positive count
    sane = Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx))
    X = Film(W, H, fill=rng)
    X.copy_pixels_from(sane, touched)
    source = Film(W, H).accumulate(gpu, rng, rng.integers(1, 4, npx))
    px = np.concatenate([np.repeat(touched, rng.integers(1, 4, touched.size)), np.repeat(barren, 2), touched[::5]])
    carries_nothing = np.concatenate([np.zeros(px.size - barren.size * 2 - touched[::5].size, bool), np.ones(barren.size * 2 + touched[::5].size, bool)])
    n_dead = 40
    px = np.concatenate([px, np.array([-1, npx], np.int64)[np.arange(n_dead) % 2]])
    carries_nothing = np.concatenate([carries_nothing, np.zeros(n_dead, bool)])
    perm = rng.permutation(px.size)
    px, carries_nothing = px[perm], carries_nothing[perm]
    d_px = dev(px.astype(np.int32))
    states = source.gather(gpu, d_px)
    for s in states:                                                           # n = 0 or -3 and garbage in every field
        junk = rng.integers(-2 ** 31, 2 ** 31, size=tuple(s.shape), dtype=np.int64).astype(np.int32)
        junk[:, 0] = np.where(rng.random(px.size) < 0.5, 0, -3)
        s[dev(carries_nothing)] = dev(junk)[dev(carries_nothing)]
    torch.cuda.synchronize()
    assert all(int((s[:, 0] == -3).sum()) > 0 and int((s[:, 0] > 0).sum()) > 0 for s in states)
    before = X.snapshot()
    runs = []
    for run in range(2):
        Y = X.copy()
        Y.combine(gpu, d_px, states)
        runs.append(Y.snapshot())
    same(runs[0], runs[1], "second run:")
    m = px.size // 2 + 1
    Z = X.copy()
    Z.combine(gpu, d_px[:m].contiguous(), [s[:m].contiguous() for s in states])
    Z.combine(gpu, d_px[m:].contiguous(), [s[m:].contiguous() for s in states])
    same(Z.snapshot(), runs[0], "two calls:")
    keep = np.ones(npx, bool)
    keep[touched] = False
    assert keep.sum() > npx // 3 and keep[barren].all()
    changed = 0
    for a, b in zip(runs[0], before):
        a, b = a.reshape(npx, -1), b.reshape(npx, -1)
        assert np.array_equal(a[keep], b[keep])
        changed += int((a[~keep] != b[~keep]).sum())
    assert changed > touched.size


# ---------------------------------------------------------------- 5. the split
def split_chunk(cnt, slot, lanes=64):
    L = (cnt + lanes - 1) // lanes
    lo, hi = min(slot * L, cnt), min((slot + 1) * L, cnt)
    return lo, hi - lo


@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_split_equals_its_construction_from_public_entries(gpu, film):
    """One pixel gets 300 records and another 65, every other pixel 0 .. 3.  split_above = 64 equals: the chunk rule, a sequential
    combine_records per chunk into the stored (slot 0) / zeroed (slots 1 .. 63) images, then 63 two-part statmc_combine_statistics
    calls in tree order.  Pixels at or below the threshold hold the sequential entry's bits; a threshold no run exceeds and
    INT32_MAX are the sequential entry everywhere."""
    import torch
    W, H = film
    npx = W * H
    rng = np.random.default_rng(500 + W)
    long_px = {63: 300, npx - 1: 65}                                           # a wave's last lane; the film's last pixel
    F = Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx))
    counts = rng.integers(0, 4, npx)
    for p, c in long_px.items():
        counts[p] = c
    px = np.repeat(np.arange(npx, dtype=np.int64), counts)
    px = with_dead(rng, px, npx, share=0.02).astype(np.int64)
    # any state is a valid record for any pixel: record i carries the state of a random pixel of one of four source films
    sources = [Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx)) for _ in range(4)]
    from_px = dev(rng.integers(0, npx, px.size).astype(np.int32))
    pick, rows = dev(rng.integers(0, 4, px.size)), torch.arange(px.size, device="cuda:0")
    per_source = [s.gather(gpu, from_px) for s in sources]
    states = [torch.stack([per_source[k][i] for k in range(4)])[pick, rows].contiguous() for i in range(len(KINDS))]
    d_px = dev(px.astype(np.int32))

    split = F.copy()
    split.combine(gpu, d_px, states, split_above=64)
    sequential = F.copy()
    sequential.combine(gpu, d_px, states, split_above=INT32_MAX)
    for never in (300, 100000):                                                # the split kernel, no run above the threshold
        G = F.copy()
        G.combine(gpu, d_px, states, split_above=never)
        same(G.snapshot(), sequential.snapshot(), "split_above = %d:" % never)

    # the construction
    def subset(idx):
        idx = dev(np.asarray(idx, np.int64))
        return d_px[idx].contiguous(), [s[idx].contiguous() for s in states]
    is_long = np.isin(px, list(long_px))
    R = F.copy()
    R.combine(gpu, *subset(np.flatnonzero(~is_long)))
    slots = [F.copy()] + [Film(W, H) for _ in range(63)]
    runs = {p: np.flatnonzero(px == p) for p in long_px}                        # ascending record index
    assert all(runs[p].size == c for p, c in long_px.items())
    for j, S in enumerate(slots):
        idx = np.concatenate([runs[p][lo:lo + ln] for p in long_px for lo, ln in [split_chunk(runs[p].size, j)]])
        if idx.size:
            S.combine(gpu, *subset(np.sort(idx)))
    stride = 1
    while stride < 64:
        for j in range(0, 64, 2 * stride):
            slots[j].combine_dense(gpu, slots[j + stride])
        stride *= 2
    R.copy_pixels_from(slots[0], list(long_px))
    same(split.snapshot(), R.snapshot(), "split_above = 64 against its construction:")

    # at or below the threshold: the sequential entry's bits; the long pixels: the same counts, other last bits
    a, b = split.snapshot(), sequential.snapshot()
    short = np.ones(npx, bool)
    short[list(long_px)] = False
    for x, y in zip(a, b):
        assert np.array_equal(x.reshape(npx, -1)[short], y.reshape(npx, -1)[short])
    assert np.array_equal(bits(split.st[RADIANCE]["n"]), bits(sequential.st[RADIANCE]["n"]))
    m3a, m3b = bits(split.st[RADIANCE]["m3"]).reshape(npx, 3), bits(sequential.st[RADIANCE]["m3"]).reshape(npx, 3)
    assert (m3a[63] != m3b[63]).any()


# ---------------------------------------------------------------- 6. the device header
@pytest.fixture(scope="module")
def example(gpu):
    from statmc_amd import build
    build.build_tools()
    lib = C.CDLL(build.DEVICE_EXAMPLE_SO)
    lib.fold_arena_records.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.mark.parametrize("film", FILMS, ids=film_ids)
def test_records_written_by_a_renderers_kernel(gpu, example, film):
    """tools/device_accumulate_example.hip, built with hipcc's default floating-point flags: a kernel folds every pixel's arena
    samples from clear() and writes PixelStats::write_record.  Those records combined into film F equal statmc_accumulate of the
    arena into a zero film Z followed by statmc_combine_statistics(F, Z)."""
    import torch
    W, H = film
    npx, S = W * H, 5
    rng = np.random.default_rng(600 + W)
    F = Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx))
    Z = Film(W, H)
    flat = make_samples(rng, S * npx)
    arenas = [dev(s.reshape(S, H, W, -1)) for s in flat]
    records = [torch.full((npx, dwords(k)), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0") for k in KINDS]
    for i, k in enumerate(KINDS):
        gpu.check(example.fold_arena_records(k[1], k[2], k[3], W, H, arenas[i].data_ptr(), S, records[i].data_ptr(), gpu.current_stream_handle()))
    gpu.accumulate(W, H, [gpu.make_stat_type(arenas[i], Z.st[i], k[2], k[3]) for i, k in enumerate(KINDS)])
    torch.cuda.synchronize()
    lifted = Z.gather(gpu, dev(np.arange(npx, dtype=np.int32)))                # the kernel's records are the gather of Z
    for i, k in enumerate(KINDS):
        assert torch.equal(records[i], lifted[i]), k[0]
    dense = F.copy()
    dense.combine_dense(gpu, Z)
    order = rng.permutation(npx)
    F.combine(gpu, dev(order.astype(np.int32)), [r[dev(order)].contiguous() for r in records])
    same(F.snapshot(), dense.snapshot())


# ---------------------------------------------------------------- 7. streams and host layers
def test_both_entries_on_a_library_stream(gpu):
    """The same bits on a stream from statmc_stream_create as on torch's current stream."""
    import torch
    W, H = FILMS[0]
    npx = W * H
    rng = np.random.default_rng(700)
    A = Film(W, H).accumulate(gpu, rng, rng.integers(0, 4, npx))
    B = Film(W, H).accumulate(gpu, rng, rng.integers(0, 3, npx))
    pixels = dev(with_dead(rng, rng.integers(0, npx, 2000), npx))              # a pixel's records: B's state, more than once
    here = A.copy()
    want_states = B.gather(gpu, pixels)
    here.combine(gpu, pixels, want_states, split_above=2)
    lib = gpu.load()
    handle = C.c_void_p()
    gpu.check(lib.statmc_stream_create(C.byref(handle)))
    try:
        there = A.copy()
        torch.cuda.synchronize()
        states = B.gather(gpu, pixels, stream=handle)
        there.combine(gpu, pixels, states, split_above=2, stream=handle)
        gpu.check(lib.statmc_synchronize(handle))
        for s, w in zip(states, want_states):
            assert torch.equal(s, w)
        same(there.snapshot(), here.snapshot())
    finally:
        gpu.check(lib.statmc_stream_destroy(handle))


def test_film_stats_wrappers(gpu):
    """FilmStats.gather_states / combine_records: the sparse hand-over of one film's touched pixels equals combine_."""
    import torch
    from statmc_amd import film, synthetic
    W, H = 64, 32
    device = torch.device("cuda:0")
    types = ("radiance", "normal", "albedo", "depth", "materialid")
    scene = synthetic.Scene(W, H, seed=3)
    main, dense, helper = (film.FilmStats(W, H, device, types=types, fused_prepass=True) for _ in range(3))
    first = {k: v.to(device) for k, v in scene.samples(4, seed=5, features=types).items()}
    more = {k: v.to(device) for k, v in scene.samples(3, seed=6, features=types).items()}
    main.accumulate(first)
    dense.accumulate(first)
    counts = (torch.rand(H, W, device=device) < 0.3).to(torch.int32) * 3          # the helper renders 30 % of the pixels
    helper.accumulate(more, counts=counts)
    _, owners = gpu.compact_offsets(counts, cap=1, owners_capacity=W * H)         # the touched-pixel list, -1 behind its end
    main.combine_records(owners, helper.gather_states(owners))
    for f in (dense.film, helper.film):
        f.zero_()
    dense.combine_(helper)
    torch.cuda.synchronize()
    assert int((owners >= 0).sum()) == int((counts > 0).sum()) > 0
    for t in types:
        for k, v in main.state[t].items():
            if v is not None:
                assert np.array_equal(bits(v), bits(dense.state[t][k])), (t, k)
    assert np.array_equal(bits(main.mean_corr), bits(dense.mean_corr)) and np.array_equal(bits(main.disc), bits(dense.disc))


def test_estimator_gather_and_combine_leave_the_c_entries_bits(gpu):
    """C++ host: Estimator::GatherStates / CombineRecords against statmc_gather_states / statmc_combine_records on the same
    descriptors, and against CombineStatistics (tests/cpp/test_state_records.cpp)."""
    from statmc_amd import build
    build.build_tools()
    out = subprocess.run([build.STATE_BIN, "61", "37"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "state records ok" in out.stdout
