"""Every accumulation entry of include/statmc.h on a set-up device, through the C ABI itself: what the entries check behind
the device -- each descriptor rule, the row ranges, the no-ops, the counted entry's compaction -- and what
statmc_debug_last_accumulate_counted reports, for every entry and not for statmc_accumulate alone.  (What they refuse ahead of
the device, alignment included: tests/test_accumulate_entries_cpu.py.  What they compute: the bit contracts of their own files.)

Every pointer of every call is a real allocation large enough for the film, so a call that is wrongly accepted folds valid
memory and fails an assertion.  All state images lie in one int32 buffer, compared bitwise as a whole."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILMS = [(16, 8), (12, 5)]           # 4-pixel groups throughout (the vector paths); rows of 12 pixels, 60 in all
S = 2                                # the capacity of every arena
F32 = 0
PLANES = ["n", "mean", "m2", "m3", "film_mean", "film_m2", "mean_corr", "discriminator"]
FILM_ENTRIES = ["statmc_accumulate", "statmc_accumulate_rows", "statmc_accumulate_row_ranges", "statmc_accumulate_formats", "statmc_accumulate_counted"]
TILE_ENTRIES = ["statmc_accumulate_tiles", "statmc_accumulate_tiles_formats", "statmc_accumulate_tiles_counted"]
RECORD_ENTRIES = ["statmc_accumulate_records", "statmc_accumulate_records_split", "statmc_accumulate_records_interleaved",
                  "statmc_accumulate_records_interleaved_split"]
ENTRIES = FILM_ENTRIES + TILE_ENTRIES + RECORD_ENTRIES
RANGED = FILM_ENTRIES[2:]
# (channels, transform, max_moment): the RGB radiance type with its epilogue, a 1-channel mean-only type, and a second one for the
# counted entry's compaction
KINDS = [(3, 1, 3), (1, 0, 1), (1, 0, 1)]


class Film:
    """One film's state (every plane of every type, whether the type's moments ask for it or not), arenas and descriptors."""

    def __init__(self, api, W, H):
        import torch
        self.api, self.lib, self.W, self.H, self.npx = api, api.load(), W, H, W * H
        rng = np.random.default_rng(100 + W)
        sizes = [(self.npx if p == "n" else self.npx * c) for c, _, _ in KINDS for p in PLANES]
        init = rng.random(sum(sizes)).astype(np.float32).view(np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)])[:-1].reshape(len(KINDS), len(PLANES))
        for t in range(len(KINDS)):
            init[self.offsets[t, 0]:self.offsets[t, 0] + self.npx] = 3          # n
        self.init = torch.from_numpy(init).cuda()
        self.state = self.init.clone()
        assert self.state.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in sizes)
        # one arena per type serves every layout: [S][H][W][C] film-major = one whole-film tile of S planes = S x npx records in
        # plane order, record r of pixel r % npx
        self.samples = [torch.from_numpy(np.exp(rng.normal(0.0, 1.0, (S, H, W, c))).astype(np.float32)).cuda() for c, _, _ in KINDS]
        self.counts = torch.full((H, W), S, dtype=torch.int32, device="cuda:0")
        self.tile_bounds = torch.tensor([0, 0, W, H], dtype=torch.int32, device="cuda:0")
        self.tile_offsets = torch.zeros(1, dtype=torch.int64, device="cuda:0")
        self.tile_samples = torch.tensor([S], dtype=torch.int32, device="cuda:0")
        px = np.tile(np.arange(self.npx, dtype=np.int32), S)
        self.pixels = torch.from_numpy(px).cuda()
        rec, self.layout = api.pack_records(px, [self.samples[t].cpu().numpy().reshape(S * self.npx, KINDS[t][0]) for t in range(2)])
        self.records = torch.from_numpy(rec).cuda()

    def plane(self, t, name):
        return self.state.data_ptr() + 4 * int(self.offsets[t, PLANES.index(name)])

    def types(self, which=(0, 1), **change):
        """Valid descriptors of the types `which`; change = {field: (index into which, value)} spoils one."""
        arr = (self.api.StatType * 17)()
        for i, t in enumerate(which):
            c, transform, mm = KINDS[t]
            d = arr[i]
            d.channels, d.transform, d.max_moment, d.n_samples = c, transform, mm, S
            d.samples, d.n, d.mean = self.samples[t].data_ptr(), self.plane(t, "n"), self.plane(t, "mean")
            d.m2 = self.plane(t, "m2") if mm >= 2 else None
            d.m3 = self.plane(t, "m3") if mm >= 3 else None
            d.film_mean, d.film_m2 = (self.plane(t, "film_mean"), self.plane(t, "film_m2")) if transform else (None, None)
            if mm == 3:
                d.mean_corr, d.discriminator = self.plane(t, "mean_corr"), self.plane(t, "discriminator")
        for field, (i, value) in change.items():
            setattr(arr[i], field, value)
        return arr

    def call(self, entry, types, n_types=2, ranges=None, n_ranges=None, n_tiles=1, n_records=None, counts=True):
        """`entry` over the whole film (or `ranges`), formats all fp32, counts all S where the entry takes them."""
        W, H, f = self.W, self.H, getattr(self.lib, entry)
        fmts = (C.c_int32 * 17)(*([F32] * 17))
        rng = (C.c_int32 * 8)(*(ranges if ranges is not None else (0, H)))
        n_ranges = n_ranges if n_ranges is not None else (len(ranges) // 2 if ranges is not None else 1)
        cnt = self.counts.data_ptr() if counts else None
        n_records = S * self.npx if n_records is None else n_records
        tiles = (self.tile_bounds.data_ptr(), self.tile_offsets.data_ptr(), self.tile_samples.data_ptr(), n_tiles)
        if entry == "statmc_accumulate":
            return f(W, H, types, n_types, None)
        if entry == "statmc_accumulate_rows":
            return f(W, H, types, n_types, rng[0], rng[1], None)
        if entry == "statmc_accumulate_row_ranges":
            return f(W, H, types, n_types, rng, n_ranges, None)
        if entry == "statmc_accumulate_formats":
            return f(W, H, types, fmts, n_types, rng, n_ranges, None)
        if entry == "statmc_accumulate_counted":
            return f(W, H, types, fmts, n_types, cnt, rng, n_ranges, None)
        if entry == "statmc_accumulate_tiles":
            return f(W, H, types, n_types, *tiles, None)
        if entry == "statmc_accumulate_tiles_formats":
            return f(W, H, types, fmts, n_types, *tiles, None)
        if entry == "statmc_accumulate_tiles_counted":
            return f(W, H, types, fmts, n_types, *tiles, cnt, None)
        tail = (8, None) if entry.endswith("_split") else (None,)
        if "interleaved" in entry:
            return f(W, H, types, n_types, self.records.data_ptr(), C.byref(self.layout), n_records, *tail)
        return f(W, H, types, n_types, self.pixels.data_ptr(), n_records, *tail)

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return torch.equal(self.state, self.init)

    def reset(self):
        self.state.copy_(self.init)

    def counts_of(self, t):
        import torch
        torch.cuda.synchronize()
        at = int(self.offsets[t, 0])
        return self.state[at:at + self.npx].cpu().numpy()


@pytest.fixture(scope="module", params=FILMS, ids=lambda f: "%dx%d" % f)
def film(request, gpu):
    return Film(gpu, *request.param)


def refusals(film):
    """(name, index of the spoilt type, the change): every descriptor rule, for the RGB type (0) and the 1-channel type (1)."""
    real = film.plane(2, "mean")        # a plane nobody else uses, for a pointer that must not be NULL
    out = []
    for i in (0, 1):
        out += [("max_moment 0", i, dict(max_moment=(i, 0))), ("max_moment 4", i, dict(max_moment=(i, 4))),
                ("transform without film_mean", i, dict(transform=(i, 1), film_mean=(i, None), film_m2=(i, real))),
                ("transform without film_m2", i, dict(transform=(i, 1), film_mean=(i, real), film_m2=(i, None))),
                ("mean_corr alone", i, dict(max_moment=(i, 3), m2=(i, real), m3=(i, real), mean_corr=(i, real), discriminator=(i, None))),
                ("discriminator alone", i, dict(max_moment=(i, 3), m2=(i, real), m3=(i, real), mean_corr=(i, None), discriminator=(i, real))),
                ("epilogue with max_moment 2", i, dict(max_moment=(i, 2), m2=(i, real), mean_corr=(i, real), discriminator=(i, real)))]
        out += [("no m2", i, dict(max_moment=(i, 2), m2=(i, None), mean_corr=(i, None), discriminator=(i, None))),
                ("no m3", i, dict(max_moment=(i, 3), m2=(i, real), m3=(i, None), mean_corr=(i, None), discriminator=(i, None)))]
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_descriptor_rule_is_enforced_by_every_entry(film, entry):
    api, lib = film.api, film.lib
    film.reset()
    for name, i, change in refusals(film):
        rc = film.call(entry, film.types(**change))
        msg = lib.statmc_last_error().decode()
        assert rc == api.ERR_INVALID, (entry, name, i, rc, msg)
        assert ("types[%d]" % i) in msg, (entry, name, i, msg)
        assert film.untouched(), (entry, name, i)


@pytest.mark.parametrize("entry", FILM_ENTRIES[1:])
def test_row_ranges_outside_reversed_and_overlapping_are_refused(film, entry):
    api, lib, H = film.api, film.lib, film.H
    film.reset()
    bad = [(0, H + 1), (-1, 2), (3, 2)]
    if entry in RANGED:
        bad += [(0, 3, 2, H), (2, H, 0, 3), (0, H, 1, 1)]
    for ranges in bad:
        rc = film.call(entry, film.types(), ranges=ranges)
        msg = lib.statmc_last_error().decode()
        assert rc == api.ERR_INVALID and "row" in msg, (entry, ranges, rc, msg)
        assert film.untouched(), (entry, ranges)
    if entry in RANGED:            # 2 types x 9 ranges: more entries than a launch holds
        rc = film.call(entry, film.types(), ranges=(0, 0, 0, 0, 0, 0, 0, 0), n_ranges=9)
        msg = lib.statmc_last_error().decode()
        assert rc == api.ERR_INVALID and "ranges" in msg, (entry, rc, msg)
        assert film.untouched(), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_nothing_to_do_is_ok_and_leaves_every_bit(film, entry):
    api = film.api
    film.reset()
    assert film.call(entry, film.types(), n_types=0) == api.STATMC_OK
    assert film.call(entry, None, n_types=0) == api.STATMC_OK
    if entry == "statmc_accumulate_row_ranges":
        assert film.call(entry, film.types(), n_ranges=0) == api.STATMC_OK
    if entry in FILM_ENTRIES[1:]:
        assert film.call(entry, film.types(), ranges=(2, 2)) == api.STATMC_OK          # an empty range
    if entry in RANGED:
        assert film.call(entry, film.types(), ranges=(0, 0, film.H, film.H)) == api.STATMC_OK
    if entry in TILE_ENTRIES:
        assert film.call(entry, film.types(), n_tiles=0) == api.STATMC_OK
    if entry in RECORD_ENTRIES:
        assert film.call(entry, film.types(), n_records=0) == api.STATMC_OK
    assert film.untouched(), entry


def test_last_accumulate_counted_follows_every_entry(film):
    """0 after an uncounted call, 1 or 2 after a counted one; the records entries leave it alone.  Every valid call folds S
    samples into every pixel of both types."""
    api, lib = film.api, film.lib
    counted = ["statmc_accumulate_counted", "statmc_accumulate_tiles_counted"]
    last = lib.statmc_debug_last_accumulate_counted
    for entry in ENTRIES:
        film.reset()
        assert film.call(counted[0], film.types()) == api.STATMC_OK and last() in (1, 2)
        before = last()
        film.reset()
        assert film.call(entry, film.types()) == api.STATMC_OK, (entry, lib.statmc_last_error())
        if entry in counted:
            assert last() in (1, 2), entry
        elif entry in RECORD_ENTRIES:
            assert last() == before, entry
        else:
            assert last() == 0, entry
        for t in (0, 1):
            assert (film.counts_of(t) == 3 + S).all(), (entry, t)
        assert (film.counts_of(2) == 3).all(), entry
    # the counted entries without counts are the uncounted ones
    for entry in counted:
        assert film.call(counted[0], film.types()) == api.STATMC_OK and last() in (1, 2)
        assert film.call(entry, film.types(), counts=False) == api.STATMC_OK and last() == 0, entry
    # a counted call resets the report before anything can refuse it
    assert film.call(counted[0], film.types()) == api.STATMC_OK and last() in (1, 2)
    assert film.call(counted[0], film.types(max_moment=(0, 4))) == api.ERR_INVALID and last() == 0


@pytest.mark.parametrize("entry", ["statmc_accumulate_counted"])
def test_a_counted_type_without_samples_is_left_out(film, entry):
    """Three types, the middle one with n_samples = 0: the bits of the call without it, and the middle type's state untouched."""
    import torch
    api = film.api
    film.reset()
    assert film.call(entry, film.types(which=(0, 2)), n_types=2) == api.STATMC_OK
    torch.cuda.synchronize()
    want = film.state.clone()
    film.reset()
    assert film.call(entry, film.types(which=(0, 1, 2), n_samples=(1, 0)), n_types=3) == api.STATMC_OK
    assert film.lib.statmc_debug_last_accumulate_counted() in (1, 2)
    torch.cuda.synchronize()
    assert torch.equal(film.state, want)
    assert (film.counts_of(1) == 3).all() and (film.counts_of(0) == 3 + S).all() and (film.counts_of(2) == 3 + S).all()
    # ... and with every type at n_samples 0 nothing is launched
    film.reset()
    assert film.call(entry, film.types(which=(0, 1), n_samples=(0, 0)), n_types=1) == api.STATMC_OK
    assert film.lib.statmc_debug_last_accumulate_counted() == 0 and film.untouched()
